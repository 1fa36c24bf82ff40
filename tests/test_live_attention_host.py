"""The host rules of the live attention ring (csts_amd/stream.py), no GPU: a pure-Python replay of the ring's frame tags under
stream_steps shows that attention_ring_slots is safe and tight, default_attention_age equals a brute-force replay of in-step
pushes, live_attention_schedule is causal, and the constructor refuses what GazeStream documents."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EGO4D = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml")
ARIA = os.path.join(ROOT, "configs/Aria/CSTS_Aria_Gaze_Forecast.yaml")


def _cfg(path):
    from csts_amd import load_yaml
    return load_yaml(path, ["NUM_GPUS", 0])


class _NoPredictor:
    """What the constructors read of a predictor before they allocate anything: its configuration."""
    def __init__(self, cfg):
        self.cfg = cfg


def _synthetic(inputs, stride, observed=30, fps=20):
    """A small forecast plan by hand: 200 / fps columns a frame, so an observed span of 30 frames holds 300 >= 257 columns."""
    inputs = np.asarray(inputs, dtype=np.int64)
    return {"segment": observed + 20, "observed": observed, "stride": stride, "clip_size": float(observed),
            "inputs": inputs, "targets": observed + np.arange(len(inputs), dtype=np.int64) * 2, "fps": Fraction(fps),
            "cols_per_frame": Fraction(200, fps)}


def _plans():
    from csts_amd import plan_stream
    return {"ego4d": (plan_stream(_cfg(EGO4D)), 32), "ego4d_stride9": (plan_stream(_cfg(EGO4D), stride=9), 32),
            "aria": (plan_stream(_cfg(ARIA)), 32), "aria_stride7": (plan_stream(_cfg(ARIA), stride=7), 16),
            "spread": (_synthetic([1, 5, 9, 13, 17, 21, 25, 29], 4), 8),        # the newer-frame bound is the larger one
            "dense": (_synthetic([22, 23, 24, 25, 26, 27, 28, 29], 8), 8)}      # the recycle bound is the larger one


PLANS = _plans()


def _patterns(plan, max_chunk, windows=6):
    """Push patterns over a recording that runs `windows` windows: {name: [(frames, samples)]}."""
    from csts_amd.stream import ring_sizes
    spf = Fraction(24000) / plan["fps"]
    assert spf.denominator == 1
    spf = int(spf)
    n = int(plan["observed"]) + windows * int(plan["stride"])
    full = int(min(plan["inputs"])) + ring_sizes(plan, max_chunk, 1)["slots"]       # what the crop ring takes before window 0 runs
    out = {"ones": [(1, spf)] * n,
           "eights": [(8, 8 * spf)] * (n // 8) + [(n % 8, n % 8 * spf)],
           "one_push": [(n, n * spf)],
           "long_then_ones": [(3 * max_chunk + 5, (3 * max_chunk + 5) * spf)] + [(1, spf)] * (n - 3 * max_chunk - 5),
           "audio_leads": [(0, max_chunk * spf)] + [(1, spf)] * n,
           # the frames run ahead until the crop ring is full, the audio catches up (windows run LATE, several in one step), and
           # from there on every chunk of frames waits for its audio
           "audio_lags": [(full, 0), (0, full * spf)] + [(max_chunk, 0), (0, max_chunk * spf)] * ((n - full) // max_chunk + 1)}
    for off in range(1, max_chunk):                              # chunks of max_chunk behind a first push of `off` frames
        out[f"chunks_after_{off}"] = [(off, off * spf)] + [(max_chunk, max_chunk * spf)] * ((n - off) // max_chunk)
    return out


def replay_ring(plan, pushes, max_chunk, max_age, Ra):
    """The ring's tags and counts under stream_steps, as csts_live_attention_add / _rows use them -> (newer, lost, rows):
    newer = writes that met a newer frame in their slot, lost = (row, frame) pairs where a frame inside a row's
    [n - max_age, n] holds fewer pairs in the ring than the windows that ran gave it, rows = [(n, known, attention_frame)]."""
    from csts_amd.stream import ring_sizes, stream_steps, stream_window
    sizes = ring_sizes(plan, max_chunk, 1)
    tag, cnt, ideal = [-1] * Ra, [0] * Ra, {}
    frames = samples = w = 0
    newer, lost, rows = [], [], []
    for k, m in pushes:
        for dk, dm, ready in stream_steps(plan, sizes["slots"], sizes["ring_cols"], max_chunk, frames, samples, w, k, m):
            for win in ready:
                for t in (int(f) for f in stream_window(plan, win)["frames_idx"]):
                    s = t % Ra
                    if tag[s] > t:
                        newer.append((win, t, tag[s]))
                    if tag[s] != t:
                        tag[s], cnt[s] = t, 0
                    cnt[s] += 1
                    ideal[t] = ideal.get(t, 0) + 1
            frames, samples, w = frames + dk, samples + dm, w + len(ready)
            for n in range(frames - dk, frames):
                span = range(n, max(0, n - max_age) - 1, -1)
                lost += [(n, j) for j in span if ideal.get(j, 0) != (cnt[j % Ra] if tag[j % Ra] == j else 0)]
                rows.append((n, w, next((j for j in span if tag[j % Ra] == j and cnt[j % Ra] > 0), -1)))
    return newer, lost, rows


@pytest.mark.parametrize("name", list(PLANS))
def test_the_ring_bound_is_safe_under_every_push_pattern(name):
    from csts_amd import attention_ring_slots, default_attention_age, live_attention_schedule
    plan, max_chunk = PLANS[name]
    for max_age in sorted({default_attention_age(plan), 0, 3}):
        Ra = attention_ring_slots(plan, max_chunk, max_age)
        spread = int(plan["inputs"][-1] - plan["inputs"][0]) - int(plan["stride"])
        assert Ra == max(1, spread + 1, max_chunk + max_age)
        patterns = _patterns(plan, max_chunk)
        for pattern in ("ones", "eights", "one_push", "long_then_ones", "audio_leads", "audio_lags", "chunks_after_5"):
            newer, lost, rows = replay_ring(plan, patterns[pattern], max_chunk, max_age, Ra)
            assert newer == [] and lost == [], (name, pattern, max_age, newer[:3], lost[:3])
            # and what the ring answers is what the schedule states on the host
            want = live_attention_schedule(plan, patterns[pattern], max_chunk=max_chunk, max_age=max_age)
            assert [(kn, g) for _, kn, g in rows] == want, (name, pattern, max_age)
            assert max(kn for _, kn, _ in rows) >= 5


def test_a_window_that_runs_late_stays_inside_the_bound():
    # the audio_lags pattern is what it says -- windows that run with many more frames in than they needed -- and the ring of
    # attention_ring_slots holds under it: a late window only writes frames that lie further below the newest one
    from csts_amd import attention_ring_slots, default_attention_age
    from csts_amd.stream import ring_sizes, stream_steps, stream_window
    plan, max_chunk = PLANS["ego4d_stride9"]
    age = default_attention_age(plan)
    newer, lost, rows = replay_ring(plan, _patterns(plan, max_chunk)["audio_lags"], max_chunk, age,
                                    attention_ring_slots(plan, max_chunk, age))
    assert newer == [] and lost == [] and any(g >= 0 for _, _, g in rows)
    sizes = ring_sizes(plan, max_chunk, 1)
    frames = samples = w = 0
    late = 0
    for k, m in _patterns(plan, max_chunk)["audio_lags"]:
        for dk, dm, ready in stream_steps(plan, sizes["slots"], sizes["ring_cols"], max_chunk, frames, samples, w, k, m):
            frames, samples, w = frames + dk, samples + dm, w + len(ready)
            late = max([late] + [frames - stream_window(plan, win)["ready_frames"] for win in ready])
    assert late >= max_chunk


@pytest.mark.parametrize("name, breaks", [("spread", "newer"), ("ego4d_stride9", "newer"), ("dense", "lost")])
def test_one_slot_fewer_breaks_the_condition_that_set_the_bound(name, breaks):
    from csts_amd import attention_ring_slots, default_attention_age
    plan, max_chunk = PLANS[name]
    max_age = default_attention_age(plan)
    Ra = attention_ring_slots(plan, max_chunk, max_age)
    spread = int(plan["inputs"][-1] - plan["inputs"][0]) - int(plan["stride"])
    assert (Ra == spread + 1) == (breaks == "newer") and (Ra == max_chunk + max_age) == (breaks == "lost")
    broken = {"newer": 0, "lost": 0}
    for pattern, pushes in _patterns(plan, max_chunk).items():
        newer, lost, _ = replay_ring(plan, pushes, max_chunk, max_age, Ra - 1)
        broken["newer"] += bool(newer)
        broken["lost"] += bool(lost)
        assert replay_ring(plan, pushes, max_chunk, max_age, Ra)[:2] == ([], []), pattern
    assert broken[breaks] > 0, broken


@pytest.mark.parametrize("name", ["ego4d", "aria", "ego4d_stride9", "aria_stride7"])
def test_default_age_is_the_smallest_that_serves_in_step_pushes(name):
    from csts_amd import default_attention_age
    plan, max_chunk = PLANS[name]
    pushes = _patterns(plan, max_chunk, windows=8)["ones"]
    age = default_attention_age(plan)
    assert age == int(plan["stride"]) - 1                       # both shipped plans end their inputs on the last observed frame
    _, _, rows = replay_ring(plan, pushes, max_chunk, 10 ** 6, 10 ** 6)      # a ring and an age that limit nothing
    first = next(n for n, kn, _ in rows if kn > 0)              # the frame whose step runs window 0
    ages = [n - g for n, _, g in rows[first:]]
    assert min(g for _, _, g in rows[first:]) >= 0 and max(ages) == age
    # with that age every frame from there on finds a map, with one less some frame does not
    assert all(g >= 0 for _, _, g in replay_ring(plan, pushes, max_chunk, age, 10 ** 6)[2][first:])
    if age > 0:
        assert any(g < 0 for _, _, g in replay_ring(plan, pushes, max_chunk, age - 1, 10 ** 6)[2][first:])


@pytest.mark.parametrize("name", ["ego4d", "ego4d_stride9", "aria"])
def test_the_schedule_is_causal(name):
    from csts_amd import live_attention_schedule, stream_live_schedule, stream_window
    plan, max_chunk = PLANS[name]
    for pattern in ("ones", "eights", "audio_lags", "one_push"):
        pushes = _patterns(plan, max_chunk)[pattern]
        rows = live_attention_schedule(plan, pushes, max_chunk=max_chunk)
        known = [kn for kn, _ in rows]
        assert known == stream_live_schedule(plan, pushes, max_chunk=max_chunk) and known == sorted(known)
        for n, (kn, g) in enumerate(rows):
            assert g <= n
            if kn == 0:
                assert g == -1
            if g >= 0:                                           # a frame some window that has run did see
                assert any(g in stream_window(plan, w)["frames_idx"] for w in range(kn))
        assert any(g >= 0 for _, g in rows)
    tight = live_attention_schedule(plan, _patterns(plan, max_chunk)["ones"], max_chunk=max_chunk, max_age=0)
    assert all(g in (-1, n) for n, (_, g) in enumerate(tight)) and any(g == n for n, (_, g) in enumerate(tight))
    with pytest.raises(ValueError, match="max_age"):
        live_attention_schedule(plan, [(1, 800)], max_age=-1)


BAD = [({"max_age": 3}, "max_age.*needs live"), ({"max_age": 3, "live": "hold"}, "max_age.*attention=True"),
       ({"max_age": 3, "attention": True}, "max_age.*needs live"),
       ({"attention_overlay": "mean", "live": "hold", "overlay": True}, "attention_overlay.*attention=True"),
       ({"attention_overlay": "mean", "attention": True}, "attention_overlay.*needs live"),
       ({"attention_overlay": "mean", "attention": True, "live": "hold"}, "pass overlay=True"),
       ({"attention_overlay": 8, "attention": True, "live": "hold", "overlay": True}, "head index in \\[0, 8\\)"),
       ({"attention_overlay": "max", "attention": True, "live": "hold", "overlay": True}, "attention_overlay must be"),
       ({"attention_overlay": True, "attention": True, "live": "hold", "overlay": True}, "attention_overlay must be"),
       ({"max_age": -1, "attention": True, "live": "hold"}, "max_age must lie in")]


@pytest.mark.parametrize("kw, word", BAD)
def test_attention_arguments_the_stream_refuses(kw, word):
    from csts_amd import GazeStream
    with pytest.raises(ValueError, match=word):
        GazeStream(_NoPredictor(_cfg(EGO4D)), **kw)


def test_capacity_and_what_is_allowed():
    from csts_amd import GazeLiveGroup, GazeStream, GazeStreamGroup
    cfg = _cfg(EGO4D)
    plain = GazeStream(_NoPredictor(cfg), live="hold")
    assert "attention_slots" not in plain.capacity and plain.attention is False and plain.max_age is None
    assert plain._attention_head is False and GazeStream(_NoPredictor(cfg), live="hold", overlay=True)._attention_head is False
    windows_only = GazeStream(_NoPredictor(cfg), attention=True)           # maps on the windows, no ring
    assert windows_only.attention and "attention_slots" not in windows_only.capacity and windows_only.capacity == GazeStream(
        _NoPredictor(cfg)).capacity
    s = GazeStream(_NoPredictor(cfg), live="linear", attention=True)
    assert s.max_age == 63 and s.capacity["attention_slots"] == 95 and s.capacity["attention_bytes"] == 95 * (9 * 64 * 4 + 12)
    assert {k: v for k, v in s.capacity.items() if not k.startswith("attention_")} == plain.capacity
    s = GazeStream(_NoPredictor(cfg), stride=9, live="hold", attention=True, overlay=True, attention_overlay=3, max_chunk=8, max_age=20)
    assert s.max_age == 20 and s.capacity["attention_slots"] == 55 and s._attention_head == 3
    assert GazeStream(_NoPredictor(cfg), live="hold", attention=True, overlay=True, attention_overlay="mean")._attention_head is None
    for make in (lambda: GazeStreamGroup(_NoPredictor(cfg), 2, attention=True), lambda: GazeLiveGroup(_NoPredictor(cfg), 2, "hold", attention=True)):
        with pytest.raises(TypeError, match="attention"):       # the groups keep refusing attention: not a keyword of theirs
            make()


def test_the_live_dict_of_no_frames_with_attention():
    from csts_amd.stream import live_empty
    plain = live_empty(64, "cpu", (48, 64))
    got = live_empty(64, "cpu", (48, 64), overlay=True, attention=(8, 8, 8), attention_overlay=True)
    extra = {"attention_frame": ((0,), torch.int64), "attention_count": ((0,), torch.int32),
             "attention_mixed": ((0, 9, 8, 8), torch.float32), "attention_maps": ((0, 9, 8, 8), torch.float32),
             "attention_range": ((0, 9, 2), torch.float32), "attention_age": ((0,), torch.int64)}
    assert list(got) == list(plain) + list(extra) + ["overlay", "attention_overlay"]
    for k, (shape, dt) in extra.items():
        assert tuple(got[k].shape) == shape and got[k].dtype == dt, k
    assert tuple(got["attention_overlay"].shape) == (0, 48, 64, 3) and got["attention_overlay"].dtype == torch.uint8
    assert "attention_overlay" not in live_empty(64, "cpu", (48, 64), overlay=True, attention=(8, 8, 8))


def test_attention_grid_of_the_shipped_configs():
    from csts_amd.infer import attention_grid
    assert attention_grid(_cfg(EGO4D)) == (8, 4, 8, 8) == attention_grid(_cfg(ARIA))
    assert attention_grid(_cfg(EGO4D), 128) == (8, 4, 4, 4)


def test_the_parser_lets_the_stream_decide_on_the_attention_flags(tmp_path, capsys):
    """The argument rules of tools/predict.py, on the tool's own parser (nothing is loaded or run)."""
    import importlib.util
    predict = os.path.join(ROOT, "tools", "predict.py")
    spec = importlib.util.spec_from_file_location("predict_tool", predict)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    base = ["--cfg", EGO4D, "--out", str(tmp_path / "o.npz"), "--video", str(tmp_path / "v.npz"), "--stream"]
    args = tool.parse_args(base + ["--attention-track"])
    assert args.attention_track and args.live is None
    args = tool.parse_args(base + ["--live", "hold", "--overlay", "--attention-overlay", "3"])
    assert args.attention_overlay == "3" and args.overlay
    assert tool.parse_args(base + ["--attention-overlay", "mean"]).attention_overlay == "mean"      # the stream refuses it, with its message
    for extra, word in ((["--attention"], "do not work with --video"), (["--fill", "hold", "--attention-track"], "not part")):
        with pytest.raises(SystemExit):
            tool.parse_args(base + extra)
        assert word in capsys.readouterr().err, extra
