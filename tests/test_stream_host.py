"""Host side of the live stream (no GPU): plan_stream / stream_window against plan_video where the two rules must agree,
stream_schedule's readiness rule, the errors, the push-splitting arithmetic of GazeStream, and the C-ABI declarations."""
import ctypes
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EGO4D = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml")
ARIA = os.path.join(ROOT, "configs/Aria/CSTS_Aria_Gaze_Forecast.yaml")
ESTIMATION = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Estimation.yaml")
ENTRY_POINTS = ("csts_stream_stft", "csts_stream_audio_windows", "csts_stream_ingest", "csts_stream_ingest_yuv", "csts_stream_gather")


def _cfg(path):
    from csts_amd import load_yaml
    return load_yaml(path, ["NUM_GPUS", 0])


# cols chosen so that cols * den == num * n for rho = 200 / fps = num / den: 30 fps -> 20 / 3, 20 fps -> 10
@pytest.mark.parametrize("yaml, n, cols, fps", [(EGO4D, 300, 2000, 30), (ESTIMATION, 300, 2000, 30), (ARIA, 300, 3000, 20)])
def test_plan_stream_agrees_with_plan_video_where_the_ratio_is_exact(yaml, n, cols, fps):
    from csts_amd import plan_stream, plan_video, stream_window
    cfg = _cfg(yaml)
    assert cfg.DATA.TARGET_FPS == fps
    for stride in (None, 9):
        video = plan_video(cfg, n, stride=stride, cols=cols)
        plan = plan_stream(cfg, stride=stride)
        assert plan["cols_per_frame"] == Fraction(200, fps) == Fraction(cols, n) and isinstance(plan["cols_per_frame"], Fraction)
        for k in ("segment", "observed", "stride", "clip_size"):
            assert plan[k] == video[k], k
        for k in ("inputs", "targets"):
            assert plan[k].dtype == np.int64 and np.array_equal(plan[k], video[k]), k
        assert video["windows"] >= 2
        for w in range(video["windows"]):
            win = stream_window(plan, w)
            assert win["frames_idx"].tolist() == video["frames_idx"][w].tolist()
            assert win["target_idx"].tolist() == video["target_idx"][w].tolist()
            assert win["audio_centers"].tolist() == video["audio_centers"][w].tolist()
            assert win["ready_frames"] == int(video["frames_idx"][w][-1]) + 1
            assert win["ready_samples"] == 120 * (int(video["audio_centers"][w].max()) + 128)


def test_ego4d_forecast_numbers():
    from csts_amd import plan_stream, plan_video, stream_window
    cfg = _cfg(EGO4D)
    video = plan_video(cfg, 300, cols=2000)
    assert video["inputs"].tolist() == [22, 31, 40, 49, 58, 67, 76, 85]
    assert video["audio_centers"][0].tolist() == [147, 207, 267, 326, 386, 444, 444, 444]
    win = stream_window(plan_stream(cfg, stride=9), 2)
    assert win["origin"] == 18 and win["frames_idx"].tolist() == [40, 49, 58, 67, 76, 85, 94, 103]
    # windows 0..2 at stride 9 share 7 of their 8 input frames with their neighbour
    w1 = stream_window(plan_stream(cfg, stride=9), 1)
    assert len(set(w1["frames_idx"].tolist()) & set(win["frames_idx"].tolist())) == 7


def test_schedule_hand_table_for_three_windows_at_stride_9():
    from csts_amd import plan_stream, stream_schedule, stream_window
    plan = plan_stream(_cfg(EGO4D), stride=9)
    # window w: o = 9 w, last input o + 85; c0 = floor(20 o / 3), c1 = floor(20 (o + 86) / 3); the last centres are clipped to
    # c1 - 129: 573 - 129 = 444, 633 - 129 = 504, 693 - 129 = 564 -> samples 120 * (centre + 128)
    table = [(86, 120 * 572), (95, 120 * 632), (104, 120 * 692)]
    for w, (frames, samples) in enumerate(table):
        win = stream_window(plan, w)
        assert (win["ready_frames"], win["ready_samples"]) == (frames, samples)
    assert stream_schedule(plan, [(85, 68640), (1, 0)]) == [[], [0]]
    assert stream_schedule(plan, [(86, 68639), (0, 1)]) == [[], [0]]
    assert stream_schedule(plan, [(104, 83039), (0, 1), (0, 0)]) == [[0, 1], [2], []]
    assert stream_schedule(plan, [(104, 83200)]) == [[0, 1, 2]]


def _emitted(plan, pushes, upto):
    from csts_amd import stream_schedule, stream_window
    out = stream_schedule(plan, pushes)
    assert len(out) == len(pushes)
    flat = [w for ws in out for w in ws]
    assert flat == list(range(upto)), flat                      # every window exactly once, in order
    cf = np.cumsum([p[0] for p in pushes])
    cs = np.cumsum([p[1] for p in pushes])
    for i, ws in enumerate(out):
        for w in ws:
            win = stream_window(plan, w)
            assert cf[i] >= win["ready_frames"] and cs[i] >= win["ready_samples"]
            assert i == 0 or cf[i - 1] < win["ready_frames"] or cs[i - 1] < win["ready_samples"]   # the FIRST such push
    return out


def test_schedule_one_frame_a_push_ragged_and_audio_ahead_or_behind():
    from csts_amd import plan_stream
    plan = plan_stream(_cfg(EGO4D), stride=9)
    n, per = 131, 800                                           # windows 0..5 need 86 + 9 w frames
    _emitted(plan, [(1, per)] * n, 6)
    rng = np.random.default_rng(0)
    cuts = sorted(rng.choice(np.arange(1, n), 17, replace=False).tolist())
    sizes = np.diff([0] + cuts + [n]).tolist()
    _emitted(plan, [(k, k * per) for k in sizes], 6)
    _emitted(plan, [(0, n * per)] + [(k, 0) for k in sizes], 6)                       # audio far ahead
    _emitted(plan, [(k, 0) for k in sizes] + [(0, 777)] * (n * per // 777 + 1), 6)    # audio far behind


def test_errors():
    from csts_amd import GazeStream, plan_stream, stream_window
    from csts_amd.stream import check_stream_rate
    cfg = _cfg(EGO4D)
    with pytest.raises(ValueError, match=r"Fraction\(30000, 1001\)"):
        plan_stream(cfg, fps=29.97)
    with pytest.raises(ValueError, match="Fraction"):
        plan_stream(cfg, fps="30")
    ntsc = plan_stream(cfg, fps=Fraction(30000, 1001))
    assert ntsc["cols_per_frame"] == Fraction(1001, 150) and stream_window(ntsc, 3)["audio_centers"].shape == (8,)
    assert plan_stream(cfg, fps=30.0)["cols_per_frame"] == plan_stream(cfg, fps=30)["cols_per_frame"] == Fraction(20, 3)
    with pytest.raises(ValueError, match="257"):
        plan_stream(cfg, fps=120)                               # 86 frames at 120 fps: 143 columns
    with pytest.raises(ValueError):
        plan_stream(cfg, stride=0)
    with pytest.raises(ValueError, match="filter state"):
        check_stream_rate(48000)
    with pytest.raises(ValueError, match="filter state"):
        GazeStream(None, sample_rate=48000)                     # refused before anything else is looked at
    assert check_stream_rate(None) == check_stream_rate(24000) == 24000


class _NoPredictor:
    """What GazeStream reads of a predictor before the first push: its configuration."""
    def __init__(self, cfg):
        self.cfg = cfg


def test_push_steps_never_overrun_a_ring_and_refuse_before_consuming():
    from csts_amd import GazeStream, stream_schedule
    from csts_amd.stream import ring_sizes
    cfg = _cfg(EGO4D)
    s = GazeStream(_NoPredictor(cfg), stride=9)
    assert s.capacity == ring_sizes(s.plan, 32, 256) == {"slots": 118, "crop_bytes": 118 * 3 * 256 * 256 * 4, "ring_cols": 832,
                                                         "spec_bytes": 256 * 832 * 4}
    # a push far longer than max_chunk: sub-chunks of at most 32 frames, the windows of stream_schedule, in order
    steps = s._steps(400, 400 * 800)
    assert sum(k for k, _, _ in steps) == 400 and sum(m for _, m, _ in steps) == 400 * 800 and max(k for k, _, _ in steps) <= 32
    assert [w for _, _, ws in steps for w in ws] == stream_schedule(s.plan, [(400, 400 * 800)])[0]
    frames = samples = 0
    done = 0
    for k, m, ws in steps:                                       # replay: no slot or column a pending window reads is overwritten
        frames, samples = frames + k, samples + m
        first = 9 * done + 22                                    # first input frame of the oldest window that has not run
        assert frames - s.R <= first and samples // 120 + 1 - s.ring_cols <= 20 * 9 * done // 3
        done += len(ws)
    with pytest.raises(ValueError, match="832 columns"):
        s._steps(0, 120 * 832)                                   # audio further ahead than the spectrum ring holds
    with pytest.raises(ValueError, match="118 slots"):
        s._steps(141, 0)                                         # frames further ahead than the crop ring holds
    assert s._steps(140, 0) == [(32, 0, []), (32, 0, []), (32, 0, []), (32, 0, []), (12, 0, [])]
    assert (s.frames, s.samples, s.next_window) == (0, 0, 0)    # planning a push consumes nothing


def test_used_frames_rule():
    from csts_amd import plan_stream
    from csts_amd.stream import used_frames
    plan = plan_stream(_cfg(EGO4D))                              # stride 64: frames 22 + 9 i + 64 w
    assert used_frames(plan, 0, 32) == [22, 31] and used_frames(plan, 86, 96) == [86, 95]
    dense = plan_stream(_cfg(EGO4D), stride=9)                   # every frame f >= 22 with f = 4 (mod 9)
    assert used_frames(dense, 0, 50) == [22, 31, 40, 49]


def test_header_declares_and_binding_binds_the_entry_points():
    from csts_amd import lib
    hdr = open(os.path.join(ROOT, "include", "csts_hip.h")).read()
    assert int(re.search(r"#define CSTS_ABI_VERSION (\d+)", hdr).group(1)) == lib.ABI_VERSION == 14
    for name in ENTRY_POINTS:
        assert name in lib.SYMBOLS and re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        for kind in ("bf16", "fp16"):
            assert hasattr(ctypes.CDLL(lib._PATHS[kind]), name), (kind, name)
    assert lib.load().csts_abi_version() == 14


def test_entry_points_reject_bad_arguments_without_a_gpu():
    from csts_amd import lib
    h = lib.load()
    fake = ctypes.c_void_p(4096)
    f3 = (ctypes.c_float * 3)(0.45, 0.45, 0.45)
    # columns [0, 2) read the samples [0, 240): a buffer of 239 does not hold them; with n_total = 239 it does
    assert h.csts_stream_stft(fake, 0, 239, -1, 0, 2, fake, 512, 511, 120, 240, 1e-6, None) == -1
    assert b"buffer does not hold" in h.csts_last_error()
    assert h.csts_stream_stft(fake, 0, 4000, -1, 0, 513, fake, 512, 511, 120, 240, 1e-6, None) == -1      # more than one turn
    assert h.csts_stream_stft(fake, 240, 4000, -1, 2, 4, fake, 512, 511, 120, 240, 1e-6, None) == -1      # column 2 reads 120..
    assert h.csts_stream_stft(fake, 0, 100, 101, 0, 1, fake, 512, 511, 120, 240, 1e-6, None) == -1        # n_total past the end
    assert h.csts_stream_audio_windows(fake, 200, 10, fake, fake, 1, 8, 256, 256, None) == -1            # width > ring_cols
    assert h.csts_stream_ingest(fake, 4, 8, 8, fake, 0, fake, fake, 12, 8, f3, f3, None) == -1           # no pair
    assert h.csts_stream_ingest(fake, 4, 8, 6001, fake, 1, fake, fake, 12, 8, f3, f3, None) == -1        # W <= 6000
    assert h.csts_stream_ingest(ctypes.c_void_p(4100), 4, 8, 8, fake, 1, fake, fake, 12, 8, f3, f3, None) == -1
    assert h.csts_stream_ingest_yuv(fake, 4, 7, 8, fake, 1, fake, fake, 12, 8, f3, f3, 1, 0, 0, None) == -1   # odd H
    assert h.csts_stream_ingest_yuv(fake, 4, 8, 8, fake, 1, fake, fake, 12, 8, f3, f3, 3, 0, 0, None) == -1   # layout
    assert h.csts_stream_gather(fake, 12, fake, fake, 1, 65, 8, None) == -1                              # T <= 64
    assert h.csts_stream_gather(fake, 0, fake, fake, 1, 8, 8, None) == -1
