"""Host side of the gaze-track fill (no GPU): infer.fill_plan against a table written out by hand, infer.default_max_gap for the
shipped YAMLs, the coverage of the default Ego4D plan after the fill, and the C-ABI symbol csts_gaze_track_fill in both
libraries with its argument checks."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EGO4D = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml")
ARIA = os.path.join(ROOT, "configs/Aria/CSTS_Aria_Gaze_Forecast.yaml")
ESTIMATION = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Estimation.yaml")
HEADER = os.path.join(ROOT, "include", "csts_hip.h")

F = 20
PREDICTED = (3, 6, 7, 16)


def _count(predicted=PREDICTED, n=F):
    c = np.zeros(n, dtype=np.int32)
    c[list(predicted)] = (1, 2, 1, 3)[:len(predicted)]
    return c


def _table(filled):
    """The neighbours written out by hand: (n, n) on predicted frames, `filled` = {frame: (a, b)}, (-1, -1) elsewhere."""
    want = np.full((F, 2), -1, dtype=np.int64)
    for n in PREDICTED:
        want[n] = (n, n)
    for n, ab in filled.items():
        want[n] = ab
    return want


def test_fill_plan_against_the_hand_table():
    from csts_amd import fill_plan
    count = _count()
    got = fill_plan(count, 4)
    assert got.dtype == np.int64 and got.shape == (F, 2)
    assert np.array_equal(got, _table({4: (3, 6), 5: (3, 6)}))
    wide = {4: (3, 6), 5: (3, 6)}
    wide.update({n: (7, 16) for n in range(8, 16)})
    assert np.array_equal(fill_plan(count, 9), _table(wide))
    assert np.array_equal(fill_plan(count, 8), _table({4: (3, 6), 5: (3, 6)}))        # 16 - 7 = 9 > 8
    assert np.array_equal(fill_plan(count, 1024), _table(wide))                        # never before the first / after the last
    for gap in (4, 9, 1024):
        got = fill_plan(count, gap)
        assert (got[:3] == -1).all() and (got[17:] == -1).all()
    assert np.array_equal(fill_plan(count, 1), _table({}))
    assert np.array_equal(fill_plan(count, 2), _table({}))                              # the closest pair with a hole is 3 apart
    assert np.array_equal(fill_plan(count, 3), _table({4: (3, 6), 5: (3, 6)}))
    with pytest.raises(ValueError):
        fill_plan(count, 0)


def test_fill_plan_without_predictions_and_on_one_frame():
    from csts_amd import fill_plan
    assert np.array_equal(fill_plan(np.zeros(F, dtype=np.int32), 9), np.full((F, 2), -1))
    assert fill_plan(np.zeros(1, dtype=np.int32), 9).tolist() == [[-1, -1]]
    assert fill_plan(np.ones(1, dtype=np.int32), 9).tolist() == [[0, 0]]
    one = np.zeros(F, dtype=np.int32)
    one[5] = 2
    want = np.full((F, 2), -1)
    want[5] = (5, 5)
    assert np.array_equal(fill_plan(one, 1024), want)                                   # one prediction has no neighbour


def test_default_max_gap_of_the_shipped_configurations():
    from csts_amd import default_max_gap, load_yaml, plan_video
    for path, n, want in ((EGO4D, 900, 9), (ARIA, 900, 5), (ESTIMATION, 900, 9)):
        cfg = load_yaml(path, ["NUM_GPUS", 0])
        plan = plan_video(cfg, n)
        assert default_max_gap(plan) == want == int(np.diff(plan["targets"]).max()), path
        assert want == cfg.DATA.SAMPLING_RATE + 1


def test_the_default_ego4d_plan_is_dense_after_the_fill():
    from csts_amd import default_max_gap, fill_plan, load_yaml, plan_video
    cfg = load_yaml(EGO4D, ["NUM_GPUS", 0])
    N = 900
    plan = plan_video(cfg, N)
    assert plan["windows"] == 13 and plan["stride"] == 64
    target = plan["target_idx"].reshape(-1)
    count = np.bincount(target[target < N], minlength=N)
    assert int((count > 0).sum()) == 102
    nb = fill_plan(count, default_max_gap(plan))
    covered = np.nonzero(nb[:, 0] >= 0)[0]
    assert covered.tolist() == list(range(86, 900)) and covered.size == 814
    filled = (count == 0) & (nb[:, 0] >= 0)
    assert int(filled.sum()) == 814 - 102
    frames = np.nonzero(filled)[0]
    assert (nb[frames, 1] - nb[frames, 0] <= 9).all() and (nb[frames, 0] < frames).all() and (frames < nb[frames, 1]).all()
    assert (count[nb[frames, 0]] > 0).all() and (count[nb[frames, 1]] > 0).all()
    # a stretch nobody forecasts stays empty: twice the stride leaves 65 frames between two windows' predictions
    sparse = plan_video(cfg, N, stride=128)
    t2 = sparse["target_idx"].reshape(-1)
    c2 = np.bincount(t2[t2 < N], minlength=N)
    nb2 = fill_plan(c2, default_max_gap(sparse))
    assert (nb2[150:214] == -1).all() and (nb2[86:150] >= 0).all()


def test_both_libraries_export_the_symbol():
    from csts_amd import lib
    hdr = open(HEADER).read()
    name = "csts_gaze_track_fill"
    assert name in lib.SYMBOLS and re.search(r"\bint\s+" + name + r"\s*\(", hdr)
    assert re.search(r"#define CSTS_GAZE_FILL_MAX_GAP 1024\b", hdr)
    for kind in ("bf16", "fp16"):
        assert hasattr(ctypes.CDLL(lib._PATHS[kind]), name), kind


def test_the_entry_point_rejects_bad_arguments_without_a_gpu():
    from csts_amd import lib
    h = lib.load()
    hdr = open(HEADER).read()
    max_hw = int(re.search(r"#define CSTS_GAZE_DECODE_MAX_HW (\d+)", hdr).group(1))
    cap = int(re.search(r"#define CSTS_GAZE_FILL_MAX_GAP (\d+)", hdr).group(1))
    maps, count, out = ctypes.c_void_p(4096), ctypes.c_void_p(8192), ctypes.c_void_p(1 << 20)

    def call(heat=maps, cnt=count, F=4, H=64, W=64, mode=1, gap=9, o=out):
        return h.csts_gaze_track_fill(heat, cnt, F, H, W, mode, gap, o, None, None, None, None, None)

    assert call(F=0) == -1
    assert b"csts_gaze_track_fill" in h.csts_last_error()
    assert call(H=1, W=max_hw + 1) == -1
    assert b"CSTS_GAZE_DECODE_MAX_HW" in h.csts_last_error()
    assert call(heat=None) == -1
    assert call(cnt=None) == -1
    assert call(mode=2) == -1
    assert call(mode=-1) == -1
    assert call(gap=0) == -1
    assert b"CSTS_GAZE_FILL_MAX_GAP" in h.csts_last_error()
    assert call(gap=cap + 1) == -1
    assert call(o=maps) == -1                                                           # in place: a frame reads its neighbours
    assert h.csts_gaze_track_fill(maps, count, 4, 64, 64, 1, 9, out, maps, None, None, None, None) == -1   # rescaled on the input
    assert h.csts_gaze_track_fill(maps, count, 4, 64, 64, 1, 9, None, None, None, None, maps, None) == -1
    assert call(o=None) == 0                                                            # nothing asked for: no launch
