"""Host side of whole-video prediction (no GPU): inputs.temporal_indices against the reference's own temporal sampling
(tests/golden/temporal_sampling.npz, written by tools/gen_golden_temporal.py from decoder.py), infer.plan_video for the three
dataset rows, its errors and audio centres, and the two new C-ABI symbols in both libraries."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "temporal_sampling.npz")
EGO4D = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml")
ARIA = os.path.join(ROOT, "configs/Aria/CSTS_Aria_Gaze_Forecast.yaml")
ESTIMATION = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Estimation.yaml")


def _cases():
    z = np.load(GOLDEN)
    return z, json.loads(str(z["cases"]))


def test_every_golden_case_reproduces_start_end_and_indices():
    from csts_amd.inputs import temporal_indices
    z, cases = _cases()
    names = [c["name"] for c in cases]
    assert len(cases) >= 30 and sum(n.startswith("random_") for n in names) == 20
    for ci, c in enumerate(cases):
        p = f"c{ci}_"
        u = float(z[p + "u"]) if c["clip_idx"] == -1 else None
        start, end, index = temporal_indices(c["video_size"], c["num_frames"], c["sampling_rate"], c["clip_idx"], c["num_clips"],
                                             target_fps=c["target_fps"], fps=c["fps"], use_offset=c["use_offset"], u=u)
        assert float(start) == float(z[p + "start"]) and float(end) == float(z[p + "end"]), (c["name"], start, end)
        assert index.dtype == np.int64 and np.array_equal(index, z[p + "index"]), (c["name"], index, z[p + "index"])
    ego = names.index("ego4d_test_clip")
    assert z[f"c{ego}_index"].tolist() == [22, 31, 40, 49, 58, 67, 76, 85]
    aria = cases[names.index("aria_T32")]
    assert (aria["video_size"], aria["num_frames"], aria["sampling_rate"]) == (60, 32, 4)
    assert int(z[f"c{names.index('aria_T32')}_index"].max()) == 59          # the clamp is active
    assert any(c["use_offset"] and c["num_clips"] == 1 for c in cases) and any(c["use_offset"] and c["num_clips"] == 3 for c in cases)
    assert any(c["fps"] != c["target_fps"] for c in cases)


def test_random_sampling_needs_its_variate():
    from csts_amd.inputs import temporal_indices
    with pytest.raises(ValueError):
        temporal_indices(86, 8, 8, -1, 1)
    with pytest.raises(ValueError):
        temporal_indices(86, 8, 8, -1, 1, u=1.0)
    with pytest.raises(ValueError):
        temporal_indices(0, 8, 8, 0, 1)
    start, end, index = temporal_indices(86, 8, 8, -1, 1, u=0.5)
    assert start == 11.0 and end == 74.0 and index.tolist() == [11, 20, 29, 38, 47, 56, 65, 74]


def test_plan_video_ego4d_forecast():
    from csts_amd import load_yaml, plan_video
    cfg = load_yaml(EGO4D, ["NUM_GPUS", 0])
    plan = plan_video(cfg, 300, stride=64)
    assert plan["windows"] == 4 and plan["segment"] == 150 and plan["observed"] == 86 and plan["stride"] == 64
    assert plan["frames_idx"].dtype == np.int32 and plan["frames_idx"].shape == (4, 8)
    assert plan["target_idx"].dtype == np.int64 and plan["target_idx"].shape == (4, 8)
    assert plan["frames_idx"][0].tolist() == [22, 31, 40, 49, 58, 67, 76, 85]
    assert plan["target_idx"][0].tolist() == [86, 95, 104, 113, 122, 131, 140, 149]
    assert plan["origins"].tolist() == [0, 64, 128, 192]
    assert np.array_equal(plan["frames_idx"], plan["origins"][:, None] + plan["inputs"][None])
    assert np.array_equal(plan["target_idx"], plan["origins"][:, None] + plan["targets"][None])
    assert int(plan["target_idx"].max()) == 192 + 149 >= 300                 # targets past the end stay in the plan
    assert "audio_centers" not in plan
    assert plan_video(cfg, 300)["stride"] == 64 and plan_video(cfg, 86)["windows"] == 1       # default: segment - observed
    assert plan_video(cfg, 86 + 63, stride=64)["windows"] == 1 and plan_video(cfg, 86 + 64, stride=64)["windows"] == 2
    # a segment override scales observed and the targets, floored
    half = plan_video(cfg, 300, segment=75)
    assert half["observed"] == 43 and half["stride"] == 32
    assert half["targets"].tolist() == [t * 75 // 150 for t in (86, 95, 104, 113, 122, 131, 140, 149)]
    assert int(half["targets"].max()) < 75 and int(half["inputs"].max()) <= 42


def test_plan_video_aria_and_estimation_rows():
    from csts_amd import load_yaml, plan_video
    from csts_amd.inputs import temporal_indices
    aria = load_yaml(ARIA, ["NUM_GPUS", 0])
    assert "aria" in aria.TEST.DATASET and aria.DATA.SAMPLING_RATE == 4 and aria.DATA.TARGET_FPS == 20
    plan = plan_video(aria, 250)
    assert (plan["segment"], plan["observed"], plan["stride"], plan["windows"]) == (100, 60, 40, 5)
    assert plan["inputs"].tolist() == temporal_indices(60, 8, 4, 1, 1, target_fps=20, fps=20)[2].tolist() == [24, 29, 34, 39, 44, 49, 54, 59]
    assert plan["targets"].tolist() == np.linspace(64, 99, 8).astype(np.int64).tolist() == [64, 69, 74, 79, 84, 89, 94, 99]
    # estimation: the Ego4D YAML with TEST.DATASET overridden, and the shipped estimation YAML
    for cfg in (load_yaml(EGO4D, ["NUM_GPUS", 0, "TEST.DATASET", "ego4d_av_gaze"]), load_yaml(ESTIMATION, ["NUM_GPUS", 0])):
        plan = plan_video(cfg, 400)
        assert (plan["segment"], plan["observed"], plan["stride"]) == (150, 150, 64)       # round(5 * 30), ceil(clip size 64)
        assert plan["windows"] == (400 - 150) // 64 + 1 == 4
        assert plan["inputs"].tolist() == [0, 9, 18, 27, 36, 45, 54, 63] and np.array_equal(plan["targets"], plan["inputs"])
        assert np.array_equal(plan["target_idx"], plan["frames_idx"].astype(np.int64))
        p25 = plan_video(cfg, 400, fps=25)
        assert p25["segment"] == 125 and p25["stride"] == 54 and p25["inputs"].tolist() == temporal_indices(125, 8, 8, 0, 1, fps=25)[2].tolist()


def test_plan_video_errors_and_audio_centres():
    from csts_amd import load_yaml, plan_video
    cfg = load_yaml(EGO4D, ["NUM_GPUS", 0])
    with pytest.raises(ValueError, match="observes 86"):
        plan_video(cfg, 85)
    with pytest.raises(ValueError):
        plan_video(cfg, 300, stride=0)
    with pytest.raises(ValueError):
        plan_video(cfg, 300, segment=1)
    # 200 frames of 24 kHz audio at hop 120: 1601 columns, 8 per frame
    plan = plan_video(cfg, 200, stride=16, cols=1601)
    assert plan["windows"] == 8
    cen = plan["audio_centers"]
    assert cen.dtype == np.int32 and cen.shape == (8, 8)
    for w, o in enumerate(plan["origins"]):
        c0, c1 = o * 1601 // 200, (o + 86) * 1601 // 200
        assert c1 - c0 >= 257 and (cen[w] >= c0 + 128).all() and (cen[w] <= c1 - 1 - 128).all()
        want = np.clip(c0 + np.rint(plan["inputs"] / 86 * (c1 - c0)).astype(np.int64), c0 + 128, c1 - 1 - 128)
        assert cen[w].tolist() == want.tolist()
    assert cen[0].tolist()[:3] == [176, 248, 320]                            # round(22 / 86 * 688) = 176: inside the clip range
    with pytest.raises(ValueError, match="257"):
        plan_video(cfg, 200, stride=16, cols=500)                            # 215 columns per window


def test_both_libraries_export_the_new_symbols():
    from csts_amd import lib
    hdr = open(os.path.join(ROOT, "include", "csts_hip.h")).read()
    for name in ("csts_clip_sample", "csts_gaze_track"):
        assert name in lib.SYMBOLS and re.search(r"\bint\s+" + name + r"\s*\(", hdr)
        for kind in ("bf16", "fp16"):
            assert hasattr(ctypes.CDLL(lib._PATHS[kind]), name), (kind, name)


def test_new_entry_points_reject_bad_arguments_without_a_gpu():
    from csts_amd import lib
    h = lib.load()
    fake = ctypes.c_void_p(4096)
    f3 = (ctypes.c_float * 3)(0.45, 0.45, 0.45)
    assert h.csts_clip_sample(fake, 0, fake, fake, fake, 1, 4, 8, 8, 8, f3, f3, None) == -1          # N >= 1
    assert b"csts_clip_sample" in h.csts_last_error()
    assert h.csts_clip_sample(fake, 7, fake, fake, fake, 1, 65, 8, 8, 8, f3, f3, None) == -1         # T <= 64
    assert h.csts_clip_sample(fake, 7, fake, fake, fake, 1, 4, 8, 6001, 8, f3, f3, None) == -1       # W <= 6000
    assert h.csts_clip_sample(fake, 7, None, fake, fake, 1, 4, 8, 8, 8, f3, f3, None) == -1
    assert h.csts_clip_sample(ctypes.c_void_p(4100), 7, fake, fake, fake, 1, 4, 8, 8, 8, f3, f3, None) == -1   # alignment
    max_hw = int(re.search(r"#define CSTS_GAZE_DECODE_MAX_HW (\d+)", open(os.path.join(ROOT, "include", "csts_hip.h")).read()).group(1))
    assert h.csts_gaze_track(fake, fake, fake, 0, 64, 64, fake, None, None, None, None, None) == -1
    assert h.csts_gaze_track(fake, fake, fake, 4, 1, max_hw + 1, fake, None, None, None, None, None) == -1
    assert b"CSTS_GAZE_DECODE_MAX_HW" in h.csts_last_error()
    assert h.csts_gaze_track(None, fake, fake, 4, 64, 64, fake, None, None, None, None, None) == -1
    assert h.csts_gaze_track(fake, fake, fake, 4, 64, 64, None, None, None, None, None, None) == 0   # nothing asked for
