"""Host side of the live track (no GPU): stream_live_schedule against a brute-force walk of GazeStream._steps, the condition that a
window whose frames were in before a push is known to that push's rows, live_ring_slots against a simulated ring, the refusals,
and the C-ABI declarations of the two kernels."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EGO4D = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml")
ARIA = os.path.join(ROOT, "configs/Aria/CSTS_Aria_Gaze_Forecast.yaml")
ESTIMATION = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Estimation.yaml")
N = 104


def _cfg(path):
    from csts_amd import load_yaml
    return load_yaml(path, ["NUM_GPUS", 0])


class _NoPredictor:
    """What GazeStream reads of a predictor before the first push: its configuration."""
    def __init__(self, cfg):
        self.cfg = cfg


def _cuts(per):
    """name -> (pushes, proportional): 104 frames and 104 * per samples, cut the ways the schedule has to survive."""
    cuts = {"one_push": ([(N, N * per)], False)}
    for k in (1, 7, 32):
        sizes = [k] * (N // k) + ([N % k] if N % k else [])
        cuts[f"pushes_of_{k}"] = ([(s, s * per) for s in sizes], True)
    fps = 24000 // per
    sizes = [1, 5, 11, 32, 2, 40, 13]
    ahead, left = [(0, fps * per)], (N - fps) * per
    for k in sizes:
        ahead.append((k, min(k * per, left)))
        left -= ahead[-1][1]
    cuts["audio_a_second_ahead"] = (ahead, False)
    rest = N - fps                  # the frames lead by a second until the last push, which brings the audio that was missing
    cuts["audio_a_second_behind"] = ([(fps, 0), (rest // 2, (rest // 2) * per),
                                      (rest - rest // 2, (rest - rest // 2 + fps) * per)], False)
    for pushes, _ in cuts.values():
        assert sum(p[0] for p in pushes) == N and sum(p[1] for p in pushes) == N * per
    return cuts


def _walk(stream, pushes):
    """The brute-force restatement: walk _steps push by push; -> (known per frame, [(first frame, frames, windows run)] per step)."""
    known, steps = [], []
    for k, m in pushes:
        for dk, dm, ready in stream._steps(k, m):
            steps.append((stream.frames, dk, list(ready)))
            stream.frames, stream.samples = stream.frames + dk, stream.samples + dm
            if ready:
                stream.next_window = ready[-1] + 1
            known += [stream.next_window] * dk
    return known, steps


CASES = [(EGO4D, 9), (EGO4D, 5), (ARIA, 9), (ARIA, 5)]


@pytest.mark.parametrize("yaml, stride", CASES)
def test_live_schedule_is_the_walk_of_the_steps(yaml, stride):
    from csts_amd import GazeStream, plan_stream, stream_live_schedule, stream_schedule, stream_window
    cfg = _cfg(yaml)
    plan = plan_stream(cfg, stride=stride)
    per = 24000 // int(plan["fps"])
    for name, (pushes, proportional) in _cuts(per).items():
        known = stream_live_schedule(plan, pushes)
        want, _ = _walk(GazeStream(_NoPredictor(cfg), stride=stride, live="linear"), pushes)
        assert known == want and len(known) == N, name
        assert all(a <= b for a, b in zip(known, known[1:])), name                  # never decreasing
        assert known[-1] == sum(len(ws) for ws in stream_schedule(plan, pushes)[:len(pushes) - (pushes[-1][0] == 0)]), name
        assert known[-1] >= 1, name                                                  # the case has a window to know about
        if proportional:        # a window whose frames were all in before the push began is known to every row of the push
            f0 = 0
            for k, _ in pushes:
                assert k <= 32
                need = 0
                while stream_window(plan, need)["ready_frames"] <= f0:
                    need += 1
                assert all(known[f] >= need for f in range(f0, f0 + k)), (name, f0)
                f0 += k
    # a smaller max_chunk cuts one push into more steps: the rows of its early frames know fewer windows
    short = stream_live_schedule(plan, [(N, N * per)], max_chunk=8)
    assert short != stream_live_schedule(plan, [(N, N * per)]) and short[-1] == known[-1]
    assert short == _walk(GazeStream(_NoPredictor(cfg), stride=stride, max_chunk=8, live="hold"), [(N, N * per)])[0]


def test_live_schedule_counts_samples_at_the_input_rate():
    from csts_amd import plan_stream, stream_live_schedule
    plan = plan_stream(_cfg(EGO4D), stride=9)
    at24 = stream_live_schedule(plan, [(13, 13 * 800)] * 8)
    assert stream_live_schedule(plan, [(13, 13 * 800)] * 8, input_rate=24000) == at24
    at48 = stream_live_schedule(plan, [(13, 13 * 1600)] * 8, input_rate=48000)
    assert len(at48) == 104 and at48[-1] == at24[-1] and all(a <= b for a, b in zip(at48, at24))   # the resampler holds samples back


def _ring_holds_what_the_rows_read(plan, steps, Rt, max_gap):
    """Replay the steps on a ring of tags: every step's windows write their targets (a differing tag is overwritten), then the rows
    of the step's frames read [f - max_gap + 1, f + max_gap - 1].  True iff every frame a row reads that some window run so far
    targets is still in its slot."""
    from csts_amd import stream_window
    tag, predicted = [-1] * Rt, set()
    for f0, dk, ready in steps:
        for w in ready:
            for t in stream_window(plan, w)["target_idx"].tolist():
                tag[t % Rt] = t
                predicted.add(t)
        for f in range(f0, f0 + dk):
            for g in range(max(0, f - max_gap + 1), f + max_gap):
                if (g in predicted) != (tag[g % Rt] == g):
                    return False
    return True


@pytest.mark.parametrize("yaml, stride", CASES)
def test_ring_slots_never_recycle_a_frame_a_row_still_reads(yaml, stride):
    from csts_amd import GazeStream, default_max_gap, live_ring_slots, plan_stream
    cfg = _cfg(yaml)
    plan = plan_stream(cfg, stride=stride)
    per = 24000 // int(plan["fps"])
    span = int(plan["targets"][-1]) - int(plan["inputs"][-1])
    for max_gap in (default_max_gap(plan), 1, 18):
        for max_chunk in (32, 8):
            Rt = live_ring_slots(plan, max_chunk, max_gap)
            assert Rt == span + max_chunk + max_gap - 1
            for name, (pushes, proportional) in _cuts(per).items():
                if max_chunk == 8 and not proportional and name != "one_push":
                    continue        # rings sized for 8-frame chunks do not hold a second of lead: the stream refuses those cuts
                s = GazeStream(_NoPredictor(cfg), stride=stride, max_chunk=max_chunk, live="linear", max_gap=max_gap)
                assert s.track_slots == Rt == s.capacity["track_slots"]
                _, steps = _walk(s, pushes)
                assert any(ws for _, _, ws in steps), name
                assert _ring_holds_what_the_rows_read(plan, steps, Rt, max_gap), (name, max_gap, max_chunk)
    # a long stream, so that the ring turns several times: 600 frames in pushes of 30, and in one push
    for pushes in ([(30, 30 * per)] * 20, [(600, 600 * per)]):
        s = GazeStream(_NoPredictor(cfg), stride=stride, live="linear")
        _, steps = _walk(s, pushes)
        assert s.next_window * stride > 3 * s.track_slots
        assert _ring_holds_what_the_rows_read(plan, steps, s.track_slots, s.max_gap)
    # the replay has teeth: a ring of three target steps, shorter than one window's target span, loses frames the rows still read
    s = GazeStream(_NoPredictor(cfg), stride=stride, live="linear")
    _, steps = _walk(s, [(N, 0), (0, N * per), (8, 8 * per)])
    assert 3 * s.max_gap < span and not _ring_holds_what_the_rows_read(plan, steps, 3 * s.max_gap, s.max_gap)
    assert _ring_holds_what_the_rows_read(plan, steps, s.track_slots, s.max_gap)


def test_ego4d_numbers_and_capacity():
    from csts_amd import GazeStream, live_ring_slots, plan_stream
    cfg = _cfg(EGO4D)
    plan = plan_stream(cfg)
    assert live_ring_slots(plan, 32, 9) == 64 + 32 + 9 - 1 == 104
    s = GazeStream(_NoPredictor(cfg), live="hold")
    assert s.max_gap == 9 and s.capacity["track_slots"] == 104 and s.capacity["track_bytes"] == 104 * (64 * 64 * 4 + 12)
    plain = GazeStream(_NoPredictor(cfg))
    assert plain.live is None and "track_slots" not in plain.capacity
    assert {k: v for k, v in s.capacity.items() if not k.startswith("track_")} == plain.capacity


def test_refusals():
    from csts_amd import GazeStream, live_ring_slots, plan_stream, stream_live_schedule
    est = _cfg(ESTIMATION)
    with pytest.raises(ValueError, match="already seen.*track_from_windows"):
        GazeStream(_NoPredictor(est), live="hold")
    with pytest.raises(ValueError, match="already seen"):
        live_ring_slots(plan_stream(est), 32, 9)
    assert GazeStream(_NoPredictor(est)).live is None                              # without live= the plan streams as before
    cfg = _cfg(EGO4D)
    with pytest.raises(ValueError, match="overlay=True.*needs live"):
        GazeStream(_NoPredictor(cfg), overlay=True)
    with pytest.raises(ValueError, match="live must be"):
        GazeStream(_NoPredictor(cfg), live="nearest")
    with pytest.raises(ValueError, match="max_gap"):
        GazeStream(_NoPredictor(cfg), max_gap=4)
    with pytest.raises(ValueError, match="max_gap must be positive"):
        GazeStream(_NoPredictor(cfg), live="hold", max_gap=0)
    with pytest.raises(ValueError, match="push_live"):
        GazeStream(_NoPredictor(cfg)).push_live()
    with pytest.raises(ValueError, match="118 slots"):                              # the push GazeStream would refuse
        stream_live_schedule(plan_stream(cfg, stride=9), [(141, 0)])


def test_header_declares_and_binding_binds_the_entry_points():
    from csts_amd import lib
    hdr = open(os.path.join(ROOT, "include", "csts_hip.h")).read()
    for name in ("csts_live_track_add", "csts_live_track_rows"):
        assert name in lib.SYMBOLS and re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        for kind in ("bf16", "fp16"):
            assert hasattr(ctypes.CDLL(lib._PATHS[kind]), name), (kind, name)
    assert int(re.search(r"#define CSTS_GAZE_FILL_MAX_GAP (\d+)", hdr).group(1)) == lib.GAZE_FILL_MAX_GAP


def test_entry_points_reject_bad_arguments_without_a_gpu():
    from csts_amd import lib
    h = lib.load()
    fake, other = ctypes.c_void_p(4096), ctypes.c_void_p(1 << 20)
    assert h.csts_live_track_add(fake, fake, 0, 64, 64, other, fake, fake, 104, None) == -1               # no map
    assert h.csts_live_track_add(fake, fake, 8, 128, 128, other, fake, fake, 104, None) == -1             # map too large
    assert h.csts_live_track_add(fake, fake, 8, 64, 64, other, fake, fake, 0, None) == -1                 # no slot
    assert h.csts_live_track_add(fake, fake, 8, 64, 64, fake, fake, fake, 104, None) == -1                # maps are the ring
    assert h.csts_live_track_add(fake, None, 8, 64, 64, other, fake, fake, 104, None) == -1
    rows = lambda *a: h.csts_live_track_rows(*a, None)                                                     # noqa: E731
    assert rows(fake, fake, fake, 104, 0, 0, 64, 64, 1, 9, other, None, None, None, None, None) == -1     # no frame
    assert rows(fake, fake, fake, 104, 0, 4, 64, 64, 2, 9, other, None, None, None, None, None) == -1     # mode
    assert rows(fake, fake, fake, 104, 0, 4, 64, 64, 1, 0, other, None, None, None, None, None) == -1     # max_gap
    assert rows(fake, fake, fake, 104, -1, 4, 64, 64, 1, 9, other, None, None, None, None, None) == -1    # f0 < 0
    assert rows(fake, fake, fake, 104, 2 ** 31 - 8, 4, 64, 64, 1, 9, other, None, None, None, None, None) == -1
    assert b"2^31" in h.csts_last_error()
    assert rows(fake, fake, fake, 104, 0, 4, 64, 64, 1, 9, fake, None, None, None, None, None) == -1      # an output is the ring
    assert rows(fake, fake, fake, 104, 0, 4, 64, 64, 1, 9, None, None, None, None, None, None) == 0       # nothing wanted: no launch
