"""The whole-recording attention track on the host: the fp32 restatement of csts_attention_track's mean
(tests/attention_track_reference.py) against float64, the end-pixel extrema against the whole lattice on AVERAGED maps, the
default fill gap, the library's exports and the command line's argument rules.  No GPU."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import attention_reference as A  # noqa: E402
import attention_track_reference as R  # noqa: E402

NAMES = sorted(R.CASES)


def float64_mean(column, idx, n_frames):
    """The rule in float64 with numpy's own mean: head mean, time mix, mean over the pairs."""
    c = np.asarray(column, dtype=np.float64)
    cols = np.concatenate([c, c.mean(axis=1, keepdims=True)], axis=1)
    T = idx.shape[1]
    mixed = A.mix_time(cols, T)                                           # (Wn, Hh + 1, T, h, w)
    out = np.zeros((n_frames,) + mixed.shape[1:2] + mixed.shape[3:])
    for f, pairs in enumerate(R.pair_lists(idx, n_frames)):
        if len(pairs):
            out[f] = np.mean([mixed[p // T, :, p % T] for p in pairs], axis=0)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_restated_mean_equals_a_float64_mean(name):
    F = R.CASES[name][8]
    col, idx = R.host_column(name), R.frames_idx(name)
    mixed, count = R.mean_maps(col, idx, F)
    want = float64_mean(col, idx, F)
    assert mixed.dtype == np.float32 and count.dtype == np.int32
    hit = count > 0
    assert 0 < int(hit.sum()) < F or name == "shipped"
    err = float((np.abs(mixed[hit].astype(np.float64) - want[hit]) / np.abs(want[hit])).max())
    print(f"attention track {name}: fp32 restatement against float64, max relative error {err:.3e}")
    assert err <= 1e-6
    assert float(np.abs(mixed[~hit]).max(initial=0.0)) == 0.0
    flat = idx.reshape(-1)
    assert np.array_equal(count, np.bincount(flat[(flat >= 0) & (flat < F)], minlength=F))


def test_the_first_case_holds_what_it_is_there_for():
    Wn, Hh, _, Tp, h, w, T, S, F, _, _ = R.CASES["grid_6x6"]
    idx = R.frames_idx("grid_6x6")
    _, count = R.mean_maps(R.host_column("grid_6x6"), idx, F)
    assert set(count.tolist()) == {0, 1, 2, 3}
    assert (idx == -1).sum() == 1 and (idx >= F).sum() == 1
    order, offsets = R.order_offsets(idx, F)
    assert offsets[1] == 0 and offsets[-1] == offsets[-2] == Wn * T - 2          # empty runs at both ends, two pairs dropped
    assert sorted(order.tolist()) == list(range(Wn * T))
    # the time axis of T' = 3 under T = 6: both clamps and the weights 1/4, 3/4
    assert [R.time_axis(j, T, Tp) for j in range(T)] == [(0, 1, 0.0), (0, 1, 0.25), (0, 1, 0.75), (1, 2, 0.25), (1, 2, 0.75),
                                                          (2, 2, 0.25)]


@pytest.mark.parametrize("name", ["grid_6x6", "grid_5x5", "shipped"])
def test_end_pixels_equal_the_whole_lattice_on_averaged_maps(name):
    """6x6 -> 48, 5x5 -> 40 and 8x8 -> 256: a mean of maps is a map, and its bilinear upsample is extremal at the end pixels."""
    S, F = R.CASES[name][7], R.CASES[name][8]
    mixed, count = R.mean_maps(R.host_column(name), R.frames_idx(name), F)
    assert int((count > 1).sum()) > 0
    m = mixed[count > 0].astype(np.float64)
    full = np.stack(A.lattice_range(m, S), axis=-1)
    assert np.array_equal(R.lattice_extrema(m, S), full)


def test_default_attention_gap_of_the_shipped_plans():
    from csts_amd import default_attention_gap, plan_video
    from csts_amd.config import load_yaml
    for yaml, gap in (("configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml", 9), ("configs/Aria/CSTS_Aria_Gaze_Forecast.yaml", 5)):
        cfg = load_yaml(os.path.join(ROOT, yaml), ["NUM_GPUS", 1])
        plan = plan_video(cfg, 400)
        assert default_attention_gap(plan) == gap == int(np.diff(plan["inputs"]).max())
    assert default_attention_gap({"inputs": np.array([3])}) == 1
    assert default_attention_gap({"inputs": np.array([3, 3, 3])}) == 1


def test_library_exports_and_binds_the_entries():
    from csts_amd import lib
    handle = lib.load()
    with open(os.path.join(ROOT, "include", "csts_hip.h")) as f:
        hdr = f.read()
    for name in ("csts_attention_track", "csts_attention_rescale"):
        assert name in lib.SYMBOLS and hasattr(handle, name)
        assert re.search(r"\bint " + name + r"\(", hdr)
    for name, value in (("GAZE_DECODE_MAX_HW", lib.GAZE_DECODE_MAX_HW), ("AUDIO_PIXEL_MAX_SIDE", lib.AUDIO_PIXEL_MAX_SIDE),
                        ("AUDIO_PIXEL_MAX_HW", lib.AUDIO_PIXEL_MAX_HW)):
        assert int(re.search(r"#define CSTS_" + name + r" (\d+)", hdr).group(1)) == value
    import csts_amd
    assert csts_amd.attention_track is csts_amd.ops.attention_track
    assert csts_amd.attention_rescale is csts_amd.ops.attention_rescale
    assert csts_amd.fill_attention_track is csts_amd.infer.fill_attention_track


def _cli(tmp_path, *flags):
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "predict.py"), *flags, "--out", str(tmp_path / "o.npz")],
                          cwd=ROOT, capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("flags", [("--attention-track",), ("--attention-overlay", "mean"), ("--attention-track", "--clip", "x")])
def test_cli_refuses_the_attention_track_without_a_recording(tmp_path, flags):
    p = _cli(tmp_path, *flags)
    assert p.returncode != 0 and p.stdout.strip() == ""
    assert "--attention-track" in p.stderr and "--video" in p.stderr
    assert not (tmp_path / "o.npz").exists()


def test_cli_refuses_a_head_that_is_no_head(tmp_path):
    p = _cli(tmp_path, "--video", "x", "--attention-overlay", "left")
    assert p.returncode != 0 and "--attention-overlay" in p.stderr and not (tmp_path / "o.npz").exists()


def test_cli_still_refuses_the_per_clip_arrays_on_a_recording(tmp_path):
    for flags in (("--attention",), ("--attention-dir", "d"), ("--attention", "--attention-track")):
        p = _cli(tmp_path, *flags, "--video", "x")
        assert p.returncode != 0 and p.stdout.strip() == ""
        assert "--attention" in p.stderr and "--video" in p.stderr and "not defined yet" in p.stderr
        assert "--attention-track" in p.stderr
        assert not (tmp_path / "o.npz").exists()
