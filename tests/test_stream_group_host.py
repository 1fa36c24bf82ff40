"""Host side of the stream group (no GPU): group_schedule's tick rule against stream_schedule and stream_steps, the refusal of a
stuck slot, the C-ABI declarations of the four group entry points and the refusals csts_group_stft and csts_group_ingest make from
the host copy of their job table, before anything is launched."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EGO4D = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml")
ENTRY_POINTS = ("csts_group_stft", "csts_group_audio_windows", "csts_group_ingest", "csts_group_ingest_yuv")
PER = 800                                                        # 24 kHz samples per frame at 30 fps


@pytest.fixture(scope="module")
def plan():
    from csts_amd import load_yaml, plan_stream
    return plan_stream(load_yaml(EGO4D, ["NUM_GPUS", 0]), stride=9)


def test_one_slot_is_stream_schedule_cut_into_groups_of_batch(plan):
    from csts_amd import group_schedule, stream_schedule
    pushes = [(8, 8 * PER)] * 16 + [(3, 0), (0, 3 * PER)]          # 131 frames: windows 0..5
    want = stream_schedule(plan, pushes)
    assert [w for ws in want for w in ws] == list(range(6))
    for batch in (1, 2, 4):
        got = group_schedule(plan, [{0: p} for p in pushes], batch)
        assert len(got) == len(pushes)
        for ws, batches in zip(want, got):                         # a push of at most max_chunk frames is one step, one round
            assert batches == [[(0, w) for w in ws[g:g + batch]] for g in range(0, len(ws), batch)]
    # everything at once: the push is worked off in steps of 32 frames, and every step's windows form their own groups
    from csts_amd.stream import ring_sizes, stream_steps
    sizes = ring_sizes(plan, 32, 1)
    steps = stream_steps(plan, sizes["slots"], sizes["ring_cols"], 32, 0, 0, 0, 131, 131 * PER)
    assert [ws for _, _, ws in steps if ws] == [[0, 1], [2, 3, 4], [5]]        # after 96, 128 and 131 frames
    assert group_schedule(plan, [{0: (131, 131 * PER)}], 2) == [[[(0, 0), (0, 1)], [(0, 2), (0, 3)], [(0, 4)], [(0, 5)]]]
    assert group_schedule(plan, [{0: (131, 131 * 1600)}], 2, input_rate=48000)[0][0] == [(0, 0), (0, 1)]


def test_three_slots_pushed_unevenly_keep_slot_window_order_and_never_mix_rounds(plan):
    from csts_amd import group_schedule
    from csts_amd.stream import ring_sizes, stream_steps
    sizes = ring_sizes(plan, 32, 1)
    # tick 0: slot 1 audio only; tick 1: slot 2 frames only; tick 2: slot 0 eight times max_chunk at once (256 frames with their
    # audio: steps of 32), slot 1 its frames (104), slot 2 its audio
    ticks = [{1: (0, 104 * PER)}, {2: (104, 0)}, {2: (0, 104 * PER), 0: (256, 256 * PER), 1: (104, 0)}]
    got = group_schedule(plan, ticks, 2)
    assert got[0] == [] and got[1] == []
    steps = {0: stream_steps(plan, sizes["slots"], sizes["ring_cols"], 32, 0, 0, 0, 256, 256 * PER),
             1: stream_steps(plan, sizes["slots"], sizes["ring_cols"], 32, 0, 104 * PER, 0, 104, 0),
             2: stream_steps(plan, sizes["slots"], sizes["ring_cols"], 32, 104, 0, 0, 0, 104 * PER)}
    assert len(steps[0]) == 8 and len(steps[1]) == 4 and len(steps[2]) == 1
    assert steps[2] == [(0, 104 * PER, [0, 1, 2])]                 # slot 2's windows are all ready in round 0
    want = []
    for r in range(8):
        rows = [(i, w) for i in (0, 1, 2) if r < len(steps[i]) for w in steps[i][r][2]]
        assert rows == sorted(rows)
        want += [rows[g:g + 2] for g in range(0, len(rows), 2)]
    assert got[2] == want
    flat = [row for b in got[2] for row in b]
    assert sorted(flat) == [(0, w) for w in range(19)] + [(1, w) for w in range(3)] + [(2, w) for w in range(3)]
    assert got[2][0] == [(2, 0), (2, 1)] and got[2][1] == [(2, 2)]      # round 0: a short batch, not filled from round 1
    assert got[2][2:4] == [[(0, 0), (0, 1)], [(1, 0), (1, 1)]]       # round 2 (96 frames): slot 0 before slot 1, cut two by two
    assert got[2][4:6] == [[(0, 2), (0, 3)], [(0, 4), (1, 2)]]       # round 3 (128 frames): one batch holds rows of two slots
    assert all(1 <= len(b) <= 2 for b in got[2])


def test_a_stuck_slot_raises_naming_the_slot_and_counts_for_nothing(plan):
    from csts_amd import group_schedule
    good = [{0: (8, 8 * PER), 1: (8, 8 * PER)}] * 10
    stuck = {0: (8, 8 * PER), 1: (0, 120 * 832)}                   # slot 1: audio further ahead than its spectrum ring holds
    with pytest.raises(ValueError, match=r"^slot 1: .*832 columns"):
        group_schedule(plan, good + [stuck], 2)
    with pytest.raises(ValueError, match=r"^slot 0: .*118 slots"):
        group_schedule(plan, [{0: (141, 0), 1: (8, 8 * PER)}], 2)
    with pytest.raises(ValueError, match="slot 1"):
        group_schedule(plan, [{1: (-1, 0)}], 2)
    after = [{0: (8, 8 * PER), 1: (8, 8 * PER)}] * 3
    # the ticks up to the refused one, then legal ones: what the legal ticks alone give
    assert group_schedule(plan, good + after, 2) == group_schedule(plan, good, 2) + group_schedule(plan, good + after, 2)[10:]
    assert group_schedule(plan, good + after, 2)[10] == [[(0, 0), (1, 0)]]       # frame 86 arrives in tick 10


def test_header_declares_and_binding_binds_the_group_entry_points():
    from csts_amd import lib
    hdr = open(os.path.join(ROOT, "include", "csts_hip.h")).read()
    assert int(re.search(r"#define CSTS_ABI_VERSION (\d+)", hdr).group(1)) == lib.ABI_VERSION == 14
    for name in ENTRY_POINTS:
        assert name in lib.SYMBOLS and re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        for kind in ("bf16", "fp16"):
            assert hasattr(ctypes.CDLL(lib._PATHS[kind]), name), (kind, name)
    assert lib.load().csts_abi_version() == 14


def _table(rows):
    t = np.asarray(rows, dtype=np.int64)
    return t, t.ctypes.data


def test_group_stft_refuses_from_the_host_table_without_a_gpu():
    from csts_amd import lib
    h = lib.load()
    fake = 4096

    def call(rows, jobs=fake, rings=fake, streams=3, ring_cols=512):
        t, ptr = _table(rows)
        return h.csts_group_stft(jobs, ptr, len(rows), rings, streams, ring_cols, 511, 120, 240, 1e-6, None)

    # {buffer, s_base, m, n_total, f0, f1, stream, first workgroup}
    assert call([[fake, 0, 4000, -1, 0, 2, 0, 0], [fake, 0, 4000, -1, 0, 2, 0, 2]]) == -1
    assert b"two jobs name one stream" in h.csts_last_error()
    assert call([[fake, 0, 4000, -1, 0, 2, 3, 0]]) == -1
    assert b"outside [0, streams)" in h.csts_last_error()
    assert call([[fake, 0, 4000, -1, 0, 2, -1, 0]]) == -1
    # columns [0, 2) read the samples [0, 240): a buffer of 239 does not hold them; the second job is the one at fault
    assert call([[fake, 0, 4000, -1, 0, 2, 0, 0], [fake, 0, 239, -1, 0, 2, 1, 2]]) == -1
    assert b"buffer does not hold" in h.csts_last_error()
    assert call([[fake, 240, 4000, -1, 2, 4, 0, 0]]) == -1                     # column 2 reads 120..
    assert call([[fake, 0, 100000, -1, 0, 513, 0, 0]]) == -1                   # more than one turn of the ring
    assert b"one turn" in h.csts_last_error()
    assert call([[fake, 0, 100, 101, 0, 1, 0, 0]]) == -1                       # n_total past the end
    assert call([[fake, 0, 4000, -1, 0, 2, 0, 0], [fake, 0, 4000, -1, 0, 2, 1, 3]]) == -1
    assert b"first workgroup" in h.csts_last_error()
    # the refusals come from the host table alone: the same with null device pointers
    assert call([[fake, 0, 4000, -1, 0, 2, 0, 0], [fake, 0, 4000, -1, 0, 2, 0, 2]], jobs=None, rings=None) == -1
    assert b"two jobs name one stream" in h.csts_last_error()
    assert h.csts_group_stft(fake, None, 1, fake, 3, 512, 511, 120, 240, 1e-6, None) == -1      # no host copy
    # jobs without columns are legal and launch nothing, so this returns 0 without a device
    assert call([[0, 0, 0, -1, 5, 5, 2, 0], [fake, 0, 100, -1, 0, 0, 0, 0]], jobs=None, rings=None) == 0


def test_group_ingest_and_audio_windows_refuse_bad_arguments_without_a_gpu():
    from csts_amd import lib
    h = lib.load()
    fake = 4096
    f3 = (ctypes.c_float * 3)(0.45, 0.45, 0.45)

    def call(rows, npairs=1, yuv=None, arena=fake):
        t, ptr = _table(rows)
        if yuv is None:
            return h.csts_group_ingest(fake, ptr, len(rows), fake, fake, npairs, arena, 24, 8, f3, f3, None)
        return h.csts_group_ingest_yuv(fake, ptr, len(rows), fake, fake, npairs, arena, 24, 8, f3, f3, yuv, 0, 0, None)

    # {chunk, bytes, K, H, W, row capacity}: 3 W + 30 rounded up to 16; 4:2:0: W + 30 rounded up to 16
    good = [fake, 4 * 8 * 8 * 3, 4, 8, 8, 64]
    assert call([good], npairs=0) == -1                                        # no pair
    assert call([good, [fake, 4 * 8 * 6001 * 3, 4, 8, 6001, 18048]]) == -1     # W <= 6000
    assert b"W <= 6000" in h.csts_last_error()
    assert call([good, [4100, 4 * 8 * 8 * 3, 4, 8, 8, 64]]) == -1
    assert b"16-byte aligned" in h.csts_last_error()
    assert call([[fake, 4 * 8 * 8 * 3 - 1, 4, 8, 8, 64]]) == -1
    assert b"chunk bytes" in h.csts_last_error()
    assert call([[fake, 4 * 8 * 8 * 3, 4, 8, 8, 48]]) == -1
    assert b"row capacity" in h.csts_last_error()
    assert call([good], arena=4100) == -1
    assert call([[fake, 4 * 12 * 8, 4, 8, 8, 48]], yuv=1, npairs=0) == -1
    assert call([[fake, 4 * 9 * 6, 4, 6, 6, 48]], yuv=3) == -1                 # layout
    assert call([[fake, 4 * 21 * 8 // 2, 4, 7, 8, 48]], yuv=1) == -1           # odd H
    assert b"even H, W" in h.csts_last_error()
    assert call([[fake, 4 * 12 * 8, 4, 8, 8, 64]], yuv=2) == -1                # the RGB capacity in a 4:2:0 job
    assert h.csts_group_audio_windows(fake, 3, 200, fake, fake, fake, fake, 1, 8, 256, 256, None) == -1      # width > ring_cols
    assert h.csts_group_audio_windows(fake, 0, 512, fake, fake, fake, fake, 1, 8, 256, 256, None) == -1
    assert h.csts_group_audio_windows(fake, 3, 512, None, fake, fake, fake, 1, 8, 256, 256, None) == -1
