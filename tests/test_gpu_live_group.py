"""GazeLiveGroup against what defines it.  With results_i the windows the group emitted for slot i and
known_i = group_live_schedule(...)[i], the live row of frame f of slot i is row f of
fill_track(track_from_windows(results_i[:known_i[f]], f + max_gap + 1), mode=live, max_gap), bit for bit (the unpredicted row for
known 0); the windows are those of a GazeStreamGroup on the same ticks; a group of one slot is a GazeStream(live=...); the
overlay is render_track of the pushed frames with those rows.  Random weights, bf16, the Ego4D forecast YAML, stride 9, and the
three recordings of tests/test_gpu_stream_group.py, restated: slot 0: 104 frames of 64 x 80, slot 1: 104 frames of 48 x 64,
slot 2: 95 frames of 64 x 80, 800 samples a frame.  On the host (stream_live_schedule, pushes of 1, 8 and 13 frames with their
audio): the 104-frame recordings give 1 frame predicted once (86), 1 predicted twice (95), 16 filled and 86 unpredicted, the
95-frame one 1 predicted, 8 filled and 86 unpredicted, so every row kind occurs in every slot."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from csts_amd import (GazeLiveGroup, GazePredictor, GazeStreamGroup, fill_track, group_live_schedule, inputs, ops,  # noqa: E402
                      points_to_source, stream_live_schedule, track_from_windows)
from csts_amd.config import load_yaml  # noqa: E402

DEV = torch.device("cuda:0")
YAML = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml")
ESTIMATION = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Estimation.yaml")
STRIDE, PER, S, GAP = 9, 800, 256, 9
SHAPES = [(104, 64, 80), (104, 48, 64), (95, 64, 80)]
WINDOW_KEYS = ("points", "peak", "heatmaps", "rescaled")
ROW_KEYS = ("points", "peak", "count", "neighbours", "filled", "rescaled")
LIVE_KEYS = ("frame_idx", "known", "points", "peak", "count", "neighbours", "filled", "rescaled", "points_source")


def bits(a, b):
    """Exact equality: floats by bit pattern (the NaN points of unpredicted frames included), everything else by value."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float32:
        return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    if a.dtype == torch.float64:
        return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))
    return torch.equal(a, b)


def _recording(n, H, W, seed, per=PER):
    g = torch.Generator().manual_seed(seed)
    frames = torch.randint(0, 256, (n, H, W, 3), generator=g, dtype=torch.uint8).to(DEV)
    return {"frames": frames, "wav": (0.1 * torch.randn(n * per, generator=g)).to(DEV)}


@pytest.fixture(scope="module")
def env():
    cfg = load_yaml(YAML, ["NUM_GPUS", 1, "CSTS_AMD.COMPUTE", "bf16"])
    torch.manual_seed(5)
    predictor = GazePredictor(cfg, device=DEV, graph=True)
    recs = [_recording(n, H, W, 40 + i) for i, (n, H, W) in enumerate(SHAPES)]
    return {"cfg": cfg, "predictor": predictor, "recs": recs, "plan": predictor.stream_group(1, stride=STRIDE).plan}


def _ticks(shapes, k):
    """Every slot pushes k frames and their audio per tick until its recording ends."""
    ticks = []
    for a in range(0, max(n for n, _, _ in shapes), k):
        ticks.append({i: (min(k, n - a), min(k, n - a) * PER) for i, (n, _, _) in enumerate(shapes) if a < n})
    return ticks


def _lagging_ticks():
    """Ticks of 8 frames in which the audio of slot 1 arrives one tick late: inside one tick it knows a window less."""
    ticks = _ticks(SHAPES, 8)
    late = [m for _, m in (t[1] for t in ticks)]
    for t, m in zip(ticks, [0] + late[:-1]):
        t[1] = (t[1][0], m)
    return ticks + [{1: (0, late[-1])}]


CUTS = {"even": (lambda: _ticks(SHAPES, 8), {"batch": 4}),
        "lagging": (_lagging_ticks, {"batch": 1}),
        "one_tick": (lambda: _ticks(SHAPES, 104), {"batch": 4}),          # longer than max_chunk: four rounds of 32 frames
        "chunk8": (lambda: _ticks(SHAPES, 13), {"batch": 4, "max_chunk": 8})}


def replay(group, ticks, recs, live=True):
    """Push the ticks cut from the recordings -> ({slot: all its windows}, {slot: its live dicts joined} or None)."""
    at, windows, lives = {}, {}, {}
    for tick in ticks:
        pieces = {}
        for i, (k, m) in tick.items():
            fa, sa = at.get(i, (0, 0))
            pieces[i] = (recs[i]["frames"][fa:fa + k] if k else None, recs[i]["wav"][..., sa:sa + m] if m else None)
            at[i] = (fa + k, sa + m)
        if live:
            res, rows = group.push_live(pieces)
            assert sorted(rows) == sorted(tick) == sorted(res)
            for i, (k, _) in tick.items():
                assert rows[i]["frame_idx"].tolist() == list(range(at[i][0] - k, at[i][0])) and rows[i]["known"].dtype == torch.int32
                lives.setdefault(i, []).append(rows[i])
        else:
            res = group.push(pieces)
        for i, rs in res.items():
            windows.setdefault(i, []).extend(rs)
    if not live:
        return windows, None
    return windows, {i: {k: torch.cat([r[k] for r in rs], dim=0) for k in rs[0]} for i, rs in lives.items()}


def offline_row(windows, known, f, mode, max_gap):
    """Row f of the rule: fill_track(track_from_windows(results[:known], f + max_gap + 1)), or the unpredicted row for known 0."""
    if known == 0:
        return {"points": torch.full((2,), float("nan"), device=DEV), "peak": torch.zeros((), device=DEV),
                "count": torch.zeros((), dtype=torch.int32, device=DEV), "neighbours": torch.full((2,), -1, dtype=torch.int32, device=DEV),
                "filled": torch.zeros((), dtype=torch.bool, device=DEV), "rescaled": torch.zeros(S // 4, S // 4, device=DEV)}
    track = fill_track(track_from_windows(windows[:known], f + max_gap + 1), mode=mode, max_gap=max_gap)
    return {k: track[k][f] for k in ROW_KEYS}


def check_slot(env, windows, live, known, mode, n, hw, max_gap=GAP):
    """Contract B on one slot: every row, its known, points_source; -> the kinds of rows that occurred."""
    assert live["known"].tolist() == known and live["frame_idx"].tolist() == list(range(n)) and len(known) == n
    assert tuple(live["rescaled"].shape) == (n, 64, 64)
    for f in range(n):
        want = offline_row(windows, known[f], f, mode, max_gap)
        for k in ROW_KEYS:
            assert bits(live[k][f], want[k]), (f, known[f], k)
    assert bits(live["points_source"], points_to_source(live["points"], env["predictor"]._video_params_row(*hw), S))
    return {("predicted" if c > 0 else "filled" if fl else "unpredicted") for c, fl in zip(live["count"].tolist(), live["filled"].tolist())}


@pytest.mark.parametrize("mode", ["hold", "linear"])
@pytest.mark.parametrize("cut", list(CUTS))
def test_live_rows_of_every_slot_equal_the_offline_composition(env, cut, mode):
    make, kw = CUTS[cut]
    ticks = make()
    group = env["predictor"].live_group(3, mode, stride=STRIDE, **kw)
    assert isinstance(group, GazeLiveGroup) and isinstance(group, GazeStreamGroup) and group.max_gap == GAP
    slots = 64 + kw.get("max_chunk", 32) + GAP - 1                # live_ring_slots: 104, or 80 with max_chunk 8
    assert group.track_slots == group.capacity["track_slots"] == slots and tuple(group._track["sum"].shape) == (3, slots, 64, 64)
    windows, lives = replay(group, ticks, env["recs"])
    sched = group_live_schedule(env["plan"], ticks, max_chunk=kw.get("max_chunk", 32))
    assert [[r["window"] for r in windows[i]] for i in range(3)] == [[0, 1, 2], [0, 1, 2], [0, 1]]
    assert max(int(r["target_idx"].max()) for r in windows[0]) == 167 >= slots        # ring slots were recycled
    for i, (n, H, W) in enumerate(SHAPES):
        kinds = check_slot(env, windows[i], lives[i], sched[i], mode, n, (H, W))
        assert kinds == {"predicted", "filled", "unpredicted"}, (i, kinds)
        assert all(r["stream"] == i for r in windows[i])
    if cut == "even":
        assert int(lives[0]["count"][95]) == 2 and lives[0]["neighbours"][88].tolist() == [86, 95]
        if mode == "hold":
            assert bits(lives[1]["rescaled"][88], lives[1]["rescaled"][86])
        else:
            assert not bits(lives[1]["rescaled"][88], lives[1]["rescaled"][87])
    if cut == "lagging":                                          # the same tick, the same frame number, another slot: one window less
        assert sched[0][80:88] == [1] * 8 and sched[1][80:88] == [0] * 8 and sched[0][88:96] == [2] * 8 and sched[1][88:96] == [1] * 8
    if cut == "one_tick":                                         # rounds of 32 frames: 96 frames know windows 0 and 1, the rest all
        assert sched[0] == [0] * 64 + [2] * 32 + [3] * 8 and sched[2] == [0] * 64 + [2] * 31
    if cut == "chunk8":
        assert sched[0] == stream_live_schedule(env["plan"], [(13, 13 * PER)] * 8, max_chunk=8)


def test_windows_are_those_of_a_stream_group_on_the_same_ticks(env):
    ticks = _lagging_ticks()
    live_windows, _ = replay(env["predictor"].live_group(3, "linear", stride=STRIDE, batch=2), ticks, env["recs"])
    plain = env["predictor"].stream_group(3, stride=STRIDE, batch=2)
    plain_windows, _ = replay(plain, ticks, env["recs"], live=False)
    assert not hasattr(plain, "_track") and "track_slots" not in plain.capacity
    for i in range(3):
        assert [r["window"] for r in live_windows[i]] == [r["window"] for r in plain_windows[i]] and len(live_windows[i]) >= 2
        for a, b in zip(live_windows[i], plain_windows[i]):
            assert a["target_idx"].tolist() == b["target_idx"].tolist()
            for k in WINDOW_KEYS:
                assert bits(a[k], b[k]), (i, a["window"], k)


def test_a_group_of_one_slot_is_a_live_stream(env):
    rec = env["recs"][0]
    pushes = [(13, 13 * PER)] * 8
    kw = dict(stride=STRIDE, batch=2, max_gap=12, overlay=True, alpha=0.5, radius=3)
    group = env["predictor"].live_group(1, "linear", **kw)
    windows, lives = replay(group, [{0: p} for p in pushes], [rec])
    stream = env["predictor"].stream(live="linear", **kw)
    assert group.max_gap == stream.max_gap == 12 and group.track_slots == stream.track_slots == 107
    per = {k: group.capacity[k] for k in ("track_slots", "track_bytes")}
    assert per == {k: stream.capacity[k] for k in per}
    base = env["predictor"].stream_group(1, stride=STRIDE, batch=2).capacity["total_bytes"]
    assert group.capacity["total_bytes"] == base + per["track_bytes"]
    fa = sa = 0
    want_windows, want_rows = [], []
    for k, m in pushes:
        res, rows = stream.push_live(rec["frames"][fa:fa + k], rec["wav"][sa:sa + m])
        want_windows += res
        want_rows.append(rows)
        fa, sa = fa + k, sa + m
    assert [r["window"] for r in windows[0]] == [r["window"] for r in want_windows] == [0, 1, 2]
    for a, b in zip(windows[0], want_windows):
        for k in WINDOW_KEYS:
            assert bits(a[k], b[k]), (a["window"], k)
    assert sorted(lives[0]) == sorted(want_rows[0]) == sorted(LIVE_KEYS + ("overlay",))
    for k in lives[0]:
        assert bits(lives[0][k], torch.cat([r[k] for r in want_rows], dim=0)), k
    assert int((lives[0]["count"] > 0).sum()) > 0 and int(lives[0]["filled"].sum()) > 0


@pytest.mark.parametrize("pixel_format", ["rgb24", "nv12"])
def test_overlay_is_render_track_of_each_slots_frames_with_its_rows(env, pixel_format):
    p = env["predictor"]
    recs = env["recs"][:2]                                        # 64 x 80 and 48 x 64
    fmt = {}
    if pixel_format == "nv12":
        fmt = {"pixel_format": "nv12", "matrix": "bt709", "full_range": False}
        g = torch.Generator().manual_seed(35)
        recs = [dict(r, frames=torch.randint(0, 256, (n, H * 3 // 2, W), generator=g, dtype=torch.uint8).to(DEV))
                for r, (n, H, W) in zip(recs, SHAPES)]
    group = p.live_group(2, "linear", stride=STRIDE, overlay=True, alpha=0.5, radius=3, **fmt)
    ticks = _ticks(SHAPES[:2], 13)
    _, lives = replay(group, ticks, recs)
    empty = group.push_live({0: (None, None), 1: (None, recs[1]["wav"][:0])})[1]
    plain = replay(p.live_group(2, "linear", stride=STRIDE, **fmt), ticks, recs)[1]
    for i, (n, H, W) in enumerate(SHAPES[:2]):
        live = lives[i]
        assert live["overlay"].dtype == torch.uint8 and tuple(live["overlay"].shape) == (n, H, W, 3)
        want = p.render_track(recs[i]["frames"], live, alpha=0.5, radius=3, **fmt)
        assert torch.equal(live["overlay"], want)
        rgb = inputs.yuv_to_rgb(recs[i]["frames"], **fmt) if fmt else recs[i]["frames"]
        nothing = live["neighbours"][:, 0] < 0
        assert 0 < int(nothing.sum()) < n
        assert torch.equal(live["overlay"][nothing], rgb[nothing]) and not torch.equal(live["overlay"][~nothing], rgb[~nothing])
        assert "overlay" not in plain[i]
        for k in plain[i]:                                        # drawing changes no row
            assert bits(plain[i][k], live[k]), (i, k)
        assert tuple(empty[i]["overlay"].shape) == (0, H, W, 3) and empty[i]["frame_idx"].numel() == 0
        assert tuple(empty[i]["rescaled"].shape) == (0, 64, 64) and sorted(empty[i]) == sorted(live)


def test_push_and_push_live_may_be_mixed(env):
    recs = env["recs"]
    group = env["predictor"].live_group(3, "hold", stride=STRIDE)
    first = group.push({i: (recs[i]["frames"][:90], recs[i]["wav"]) for i in range(3)})       # folded, but no frame answered
    assert [[r["window"] for r in first[i]] for i in range(3)] == [[0], [0], [0]]
    windows, live = group.push_live({i: (recs[i]["frames"][90:], None) for i in range(3)})
    sched = group_live_schedule(env["plan"], [{i: (90, n * PER) for i, (n, _, _) in enumerate(SHAPES)},
                                              {i: (n - 90, 0) for i, (n, _, _) in enumerate(SHAPES)}])
    for i, (n, H, W) in enumerate(SHAPES):
        both = first[i] + windows[i]
        assert [r["window"] for r in both] == list(range(3 if n == 104 else 2))
        assert live[i]["frame_idx"].tolist() == list(range(90, n)) and live[i]["known"].tolist() == sched[i][90:] == [len(both)] * (n - 90)
        for at, f in enumerate(range(90, n)):
            want = offline_row(both, len(both), f, "hold", GAP)
            for k in ROW_KEYS:
                assert bits(live[i][k][at], want[k]), (i, f, k)
        assert int((live[i]["count"] > 0).sum()) == (1 if n == 104 else 0) and int(live[i]["filled"].sum()) > 0      # frame 95


def test_a_reset_slot_forgets_the_previous_recording(env):
    recs = list(env["recs"])
    group = env["predictor"].live_group(3, "linear", stride=STRIDE)
    ticks = _ticks(SHAPES, 8)
    replay(group, ticks, recs)
    assert int((group._track["frame"][2] >= 0).sum()) > 0
    closing = group.close(2)
    group.reset(2)
    assert int(group._track["frame"][2].max()) == -1 and int(group._track["count"][2].sum()) == 0       # cleared on the device
    assert int((group._track["frame"][0] >= 0).sum()) > 0                                                # and only that slot
    assert closing == {2: []} and group.frames[2] == 0 and group.hw[2] is None
    # another, shorter recording of another size on the same slot: its frames 86 .. carry the tags the old recording left
    recs[2] = _recording(92, 48, 64, 77)
    shapes = [(0, 0, 0), (0, 0, 0), (92, 48, 64)]
    new_ticks = [{2: t[2]} for t in _ticks(shapes, 8)]
    windows, lives = replay(group, new_ticks, recs)
    sched = group_live_schedule(env["plan"], new_ticks)
    assert [r["window"] for r in windows[2]] == [0] and sched[2][80:88] == [1] * 8
    kinds = check_slot(env, windows[2], lives[2], sched[2], "linear", 92, (48, 64))
    assert kinds == {"predicted", "filled", "unpredicted"} and int(lives[2]["count"][86]) == 1
    with pytest.raises(ValueError, match="close\\(0\\) first"):
        group.reset(0)


def test_a_tick_is_one_rows_launch_and_at_most_one_add_launch(env, monkeypatch):
    recs = env["recs"]
    group = env["predictor"].live_group(3, "hold", stride=STRIDE)
    calls = {"add": 0, "rows": 0, "single": 0}

    def counted(name, fn):
        def wrapper(*args, **kwargs):
            calls[name] += 1
            return fn(*args, **kwargs)
        return wrapper

    monkeypatch.setattr(ops, "group_live_add", counted("add", ops.group_live_add))
    monkeypatch.setattr(ops, "group_live_rows", counted("rows", ops.group_live_rows))
    monkeypatch.setattr(ops, "live_track_add", counted("single", ops.live_track_add))
    monkeypatch.setattr(ops, "live_track_rows", counted("single", ops.live_track_rows))
    seen = []
    for t in range(11):                                           # ticks 0..9 run no window, tick 10 (frames 80..87) runs three
        a = 8 * t
        windows, live = group.push_live({i: (recs[i]["frames"][a:a + 8], recs[i]["wav"][a * PER:(a + 8) * PER]) for i in range(3)})
        seen.append((calls["add"], calls["rows"], sum(len(w) for w in windows.values())))
        assert all(live[i]["frame_idx"].tolist() == list(range(a, a + 8)) for i in range(3))
        calls["add"] = calls["rows"] = 0
    assert seen == [(0, 1, 0)] * 10 + [(1, 1, 3)] and calls["single"] == 0
    group.push_live({0: (None, recs[0]["wav"][:0])})              # no frames: nothing to answer, nothing launched
    assert (calls["add"], calls["rows"]) == (0, 0)


class _NoPredictor:
    """What GazeLiveGroup reads of a predictor before it allocates anything: its configuration."""
    def __init__(self, cfg):
        self.cfg = cfg


def test_argument_refusals(env):
    p = env["predictor"]
    with pytest.raises(ValueError, match="already seen.*track_from_windows"):
        GazeLiveGroup(_NoPredictor(load_yaml(ESTIMATION, ["NUM_GPUS", 1])), 2, "hold")
    with pytest.raises(ValueError, match="live must be one of"):
        p.live_group(2, None)
    with pytest.raises(ValueError, match="live must be one of"):
        p.live_group(2, "nearest")
    with pytest.raises(TypeError):
        p.live_group(2)                                           # live is required
    with pytest.raises(ValueError, match="alpha must lie in"):
        p.live_group(2, "hold", overlay=True, alpha=1.5)
    with pytest.raises(ValueError, match="radius"):
        p.live_group(2, "hold", overlay=True, radius=-1)
    with pytest.raises(ValueError, match="max_gap must be positive"):
        p.live_group(2, "hold", max_gap=0)
    with pytest.raises(ValueError, match="positive"):
        p.live_group(0, "hold")
    group = p.live_group(2, "hold", stride=STRIDE)
    frames = env["recs"][0]["frames"]
    group.close()
    with pytest.raises(ValueError, match="^slot 1: the stream is closed"):
        group.push_live({1: (frames[:1], None)})
    assert group._answers is None and group.frames == [0, 0]
    group.reset(1)
    windows, live = group.push_live({1: (frames[:2], None)})
    assert windows == {1: []} and live[1]["known"].tolist() == [0, 0] and live[1]["neighbours"].tolist() == [[-1, -1]] * 2
    with pytest.raises(ValueError, match="^slot 1: .*64 x 80"):
        group.push_live({1: (env["recs"][1]["frames"][:1], None)})
    assert group.frames == [0, 2]
