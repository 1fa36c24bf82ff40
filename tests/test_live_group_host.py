"""Host side of the live group (no GPU): group_live_schedule against stream_live_schedule slot by slot, the refusal of a stuck
slot, the C-ABI declarations of csts_group_live_add and csts_group_live_rows and the refusals both make before anything is
launched, called with null device pointers."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EGO4D = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml")
ENTRY_POINTS = ("csts_group_live_add", "csts_group_live_rows")
PER = 800                                                        # 24 kHz samples per frame at 30 fps


@pytest.fixture(scope="module")
def plan():
    from csts_amd import load_yaml, plan_stream
    return plan_stream(load_yaml(EGO4D, ["NUM_GPUS", 0]), stride=9)


def test_even_ticks_are_stream_live_schedule_of_every_slot(plan):
    from csts_amd import group_live_schedule, stream_live_schedule
    lengths = {0: 104, 1: 104, 2: 95}
    ticks = []
    for a in range(0, 104, 8):
        ticks.append({i: (min(8, n - a), min(8, n - a) * PER) for i, n in lengths.items() if a < n})
    got = group_live_schedule(plan, ticks)
    assert sorted(got) == [0, 1, 2]
    for i, n in lengths.items():
        pushes = [t[i] for t in ticks if i in t]
        assert sum(k for k, _ in pushes) == n
        assert got[i] == stream_live_schedule(plan, pushes) and len(got[i]) == n
    assert got[0] == got[1]
    assert got[0][:80] == [0] * 80 and got[0][80:88] == [1] * 8 and got[0][96:] == [3] * 8      # frame 86 arrives in tick 10
    assert got[2][88:] == [2] * 7                                   # window w needs 86 + 9 w frames: 95 frames run windows 0, 1


def test_uneven_ticks_max_chunk_and_input_rate_follow_each_slot_alone(plan):
    from csts_amd import group_live_schedule, stream_live_schedule
    # slot 1's audio lags: it knows fewer windows than slot 0 inside the same tick; slot 2 joins late and pushes all at once
    ticks = [{0: (40, 40 * PER), 1: (40, 20 * PER)}, {0: (50, 50 * PER), 1: (50, 30 * PER), 2: (0, 10 * PER)},
             {1: (0, 54 * PER)}, {0: (14, 14 * PER), 1: (14, 0), 2: (131, 121 * PER)}]
    for max_chunk in (32, 8):
        got = group_live_schedule(plan, ticks, max_chunk=max_chunk)
        for i in (0, 1, 2):
            pushes = [t[i] for t in ticks if i in t]
            assert got[i] == stream_live_schedule(plan, pushes, max_chunk=max_chunk), (i, max_chunk)
    got = group_live_schedule(plan, ticks)
    assert len(got[0]) == len(got[1]) == 104 and len(got[2]) == 131
    assert got[0][89] == 1 and got[1][89] == 0                      # the same frame of the same tick, another slot, another known
    assert got[2] == sorted(got[2]) and got[2][-1] == 6
    ticks48 = [{0: (13, 13 * 2 * PER), 1: (13, 13 * 2 * PER)}] * 8
    got48 = group_live_schedule(plan, ticks48, input_rate=48000)
    assert got48[0] == got48[1] == stream_live_schedule(plan, [(13, 13 * 2 * PER)] * 8, input_rate=48000)
    assert group_live_schedule(plan, []) == {}


def test_a_stuck_slot_raises_naming_the_slot_as_group_schedule_does(plan):
    from csts_amd import group_live_schedule, group_schedule
    good = [{0: (8, 8 * PER), 1: (8, 8 * PER)}] * 10
    stuck = {0: (8, 8 * PER), 1: (0, 120 * 832)}                   # slot 1: audio further ahead than its spectrum ring holds
    for ticks, pattern in ((good + [stuck], r"^slot 1: .*832 columns"), ([{0: (141, 0), 1: (8, 8 * PER)}], r"^slot 0: .*118 slots"),
                           ([{1: (-1, 0)}], "slot 1")):
        with pytest.raises(ValueError, match=pattern) as ours:
            group_live_schedule(plan, ticks)
        with pytest.raises(ValueError, match=pattern) as theirs:
            group_schedule(plan, ticks, 2)
        assert str(ours.value) == str(theirs.value)


def test_header_declares_and_binding_binds_the_live_group_entry_points():
    import csts_amd
    from csts_amd import lib
    hdr = open(os.path.join(ROOT, "include", "csts_hip.h")).read()
    assert int(re.search(r"#define CSTS_ABI_VERSION (\d+)", hdr).group(1)) == lib.ABI_VERSION
    for name in ENTRY_POINTS:
        assert name in lib.SYMBOLS and re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        for kind in ("bf16", "fp16"):
            assert hasattr(ctypes.CDLL(lib._PATHS[kind]), name), (kind, name)
    assert lib.load().csts_abi_version() == lib.ABI_VERSION
    assert len(lib.SYMBOLS["csts_group_live_add"][1]) == 12 and len(lib.SYMBOLS["csts_group_live_rows"][1]) == 19
    assert callable(csts_amd.GazeLiveGroup) and callable(csts_amd.group_live_schedule) and hasattr(csts_amd.GazePredictor, "live_group")
    assert issubclass(csts_amd.GazeLiveGroup, csts_amd.GazeStreamGroup)
    for name in ("group_live_ring", "group_live_add", "group_live_rows"):
        assert callable(getattr(csts_amd.ops, name))


def test_group_live_add_refuses_bad_arguments_without_a_gpu():
    from csts_amd import lib
    h = lib.load()
    fake = 4096

    def call(P=3, H=64, W=64, streams=3, Rt=7, maps=None, target=None, stream_of=None, sum_=None, count=None, frame=None):
        return h.csts_group_live_add(maps, target, stream_of, P, H, W, sum_, count, frame, streams, Rt, None)

    # the sizes are refused whatever the pointers are: here all null
    for kw, msg in (({"P": 0}, b"1 <= P <= 65535"), ({"P": 65536}, b"1 <= P <= 65535"), ({"Rt": 0}, b"1 <= Rt <= 65535"),
                    ({"Rt": 65536}, b"1 <= Rt <= 65535"), ({"streams": 0}, b"streams"), ({"streams": -1}, b"streams"),
                    ({"streams": 65535, "Rt": 65535}, b"streams * Rt < 2^31"), ({"H": 0}, b"H * W"),
                    ({"H": 128, "W": 65}, b"CSTS_GAZE_DECODE_MAX_HW"), ({"H": 65536, "W": 65536}, b"H * W")):
        assert call(**kw) == -1, kw
        assert msg in h.csts_last_error(), (kw, h.csts_last_error())
    full = dict(maps=fake, target=fake, stream_of=fake, sum_=2 * fake, count=fake, frame=fake)
    assert call(P=0, **full) == -1 and call(streams=0, **full) == -1
    for name in full:                                               # every pointer is needed
        assert call(**dict(full, **{name: None})) == -1, name
        assert b"null" in h.csts_last_error()
    assert call(**dict(full, sum_=fake)) == -1
    assert b"maps must not be the arena" in h.csts_last_error()


def test_group_live_rows_refuses_bad_arguments_without_a_gpu():
    from csts_amd import lib
    h = lib.load()
    fake = 4096

    def call(K=3, H=64, W=64, streams=3, Rt=7, mode=1, max_gap=9, sum_=None, count=None, frame=None, stream_of=None, frame_of=None,
             outs=(None,) * 6):
        return h.csts_group_live_rows(sum_, count, frame, streams, Rt, stream_of, frame_of, K, H, W, mode, max_gap, *outs, None)

    for kw, msg in (({"K": 0}, b"1 <= K <= 65535"), ({"K": 65536}, b"1 <= K <= 65535"), ({"Rt": 0}, b"1 <= Rt <= 65535"),
                    ({"Rt": 65536}, b"1 <= Rt <= 65535"), ({"streams": 0}, b"1 <= streams"),
                    ({"streams": 1 << 20, "Rt": 4096}, b"streams * Rt < 2^31"), ({"W": 0}, b"H * W"),
                    ({"H": 128, "W": 65}, b"CSTS_GAZE_DECODE_MAX_HW"), ({"mode": 2}, b"mode must be 0"), ({"mode": -1}, b"mode must be 0"),
                    ({"max_gap": 0}, b"max_gap"), ({"max_gap": lib.GAZE_FILL_MAX_GAP + 1}, b"CSTS_GAZE_FILL_MAX_GAP")):
        assert call(**kw) == -1, kw
        assert msg in h.csts_last_error(), (kw, h.csts_last_error())
    full = dict(sum_=2 * fake, count=3 * fake, frame=fake, stream_of=fake, frame_of=fake)
    for name in full:
        assert call(**dict(full, **{name: None})) == -1, name
        assert b"null" in h.csts_last_error()
    for at in (0, 1):                                               # heatmaps or rescaled on the sums
        outs = [None] * 6
        outs[at] = 2 * fake
        assert call(outs=tuple(outs), **full) == -1
        assert b"no output may be the arena" in h.csts_last_error()
    assert call(outs=(None, None, None, None, 3 * fake, None), **full) == -1        # out_count on the counts
    assert b"no output may be the arena" in h.csts_last_error()
    assert call(**full) == 0                                        # nothing asked for: nothing launched, no device needed
