"""Audio at any sample rate, the host side (no GPU): the float64 restatement of the rule (tests/resample_reference.py) against
scipy.signal.resample_poly / firwin, the package's own rule (inputs.resample_rule) against the restatement, ratio reduction and
output lengths, the identity case, the ValueErrors, and the C entry points: declared, exported by both libraries, and refusing
bad arguments on the CPU before any launch.

Bound of the scipy comparison: 1e-12 absolute on unit-variance input (measured 2.3e-15 with scipy 1.15.3; the margin covers
another BLAS's summation order)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import resample_reference as R  # noqa: E402
from csts_amd import inputs, lib  # noqa: E402

RATIOS = {8000: (3, 1), 11025: (320, 147), 12000: (2, 1), 16000: (3, 2), 22050: (160, 147), 32000: (3, 4), 44100: (80, 147),
          48000: (1, 2), 88200: (40, 147), 96000: (1, 4), 176400: (20, 147), 192000: (1, 8)}


@pytest.mark.parametrize("rate", R.RATES)
def test_restatement_equals_scipy(rate):
    signal = pytest.importorskip("scipy.signal")
    h, up, down, half = R.design(rate)
    fir = signal.firwin(2 * half + 1, 1.0 / max(up, down), window=("kaiser", 5.0)) * up
    assert float(np.abs(h - fir).max()) <= 1e-15 * up
    worst = 0.0
    for n in R.LENGTHS:
        x = np.random.default_rng(rate + n).standard_normal(n)
        want = signal.resample_poly(x, up, down)
        y, K, S = R.resample(x, h, up, down, half)
        assert y.shape == want.shape == (R.out_len(n, up, down),)
        worst = max(worst, float(np.abs(y - want).max()))
        assert int(K.min()) >= 1 and int(K.max()) <= 2 * half // up + 1 and bool((S >= np.abs(y) - 1e-15).all())
    print(f"{rate} Hz ({up}/{down}): restatement vs scipy.signal.resample_poly, largest difference {worst:.2e}")
    assert worst <= 1e-12


@pytest.mark.parametrize("rate", R.RATES)
def test_ratio_length_and_rule_of_the_package(rate):
    assert R.ratio(rate) == RATIOS[rate]
    h, up, down, half = inputs.resample_rule(rate)
    want, *rest = R.design(rate)
    assert (up, down, half) == tuple(rest) == RATIOS[rate] + (10 * max(RATIOS[rate]),)
    assert h.dtype == np.float64 and h.shape == (2 * half + 1,) and np.array_equal(h, want)
    assert inputs.resample_rule(rate)[0] is h                                       # cached
    assert h.size <= 6401 and inputs.resample_lds_floats(up, down, half) <= lib.RESAMPLE_MAX_LDS_FLOATS
    handle = lib.load()
    for n in R.LENGTHS + (24000 * 300, 192000 * 3600):
        assert handle.csts_resample_len(n, up, down) == R.out_len(n, up, down) == -(-n * 24000 // rate)
    # other arguments: another filter, another target
    h2, *_ = inputs.resample_rule(rate, zeros=4, beta=8.0)
    assert h2.shape == (2 * 4 * max(up, down) + 1,) and np.array_equal(h2, R.design(rate, zeros=4, beta=8.0)[0])
    assert inputs.resample_rule(24000, target_rate=rate)[1:3] == (down, up)


def test_identity_rate_is_a_delta_and_needs_no_device():
    h, up, down, half = inputs.resample_rule(24000)
    assert (up, down, half) == (1, 1, 10) and h[half] == pytest.approx(1.0, abs=1e-15)
    assert float(np.abs(np.delete(h, half)).max()) <= 1e-16
    x = np.random.default_rng(0).standard_normal(50)
    assert float(np.abs(R.resample(x, h, 1, 1, 10)[0] - x).max()) <= 1e-15


@pytest.mark.parametrize("rate", [0, -48000, 48000.0, 44100.5, "48000", None, True])
def test_bad_rates_are_value_errors(rate):
    from csts_amd import infer
    wav = torch.zeros(100)
    with pytest.raises(ValueError, match="positive integer"):
        inputs.check_sample_rate(rate)
    with pytest.raises(ValueError, match="positive integer"):
        inputs.resample_rule(rate)
    with pytest.raises(ValueError, match="positive integer"):
        inputs.resample_audio(wav, rate)                                            # refused before the device is looked at
    if rate is not None:
        with pytest.raises(ValueError, match="positive integer"):
            infer._check_video_wav(wav, rate)


def test_video_waveform_shapes_are_validated_on_the_host():
    from csts_amd import infer
    mono, stereo = torch.zeros(100), torch.zeros(2, 100)
    infer._check_video_wav(mono, None)
    infer._check_video_wav(mono, 48000)
    infer._check_video_wav(stereo, np.int64(48000))
    infer._check_video_wav(stereo.to(torch.int16), 48000)
    with pytest.raises(ValueError, match="sample_rate"):
        infer._check_video_wav(stereo, None)                                         # 2-D wav without a rate
    with pytest.raises(ValueError):
        infer._check_video_wav(mono.to(torch.int16), None)
    with pytest.raises(ValueError):
        infer._check_video_wav(torch.zeros(1, 2, 100), 48000)
    with pytest.raises(ValueError):
        infer._check_video_wav(stereo.to(torch.int32), 48000)
    with pytest.raises(ValueError):
        inputs.resample_audio(torch.zeros(1, 1, 2, 100), 48000)
    with pytest.raises(ValueError):
        inputs.resample_audio(torch.zeros(100, dtype=torch.int32), 48000)
    with pytest.raises(lib.CstsError):
        inputs.resample_audio(mono, 48000)                                           # a CPU tensor: no fallback


@pytest.mark.parametrize("rate", [24001, 47999, 44101])
def test_ratio_beyond_the_table_names_the_reduced_ratio(rate):
    up, down = R.ratio(rate)
    with pytest.raises(ValueError, match=f"{up}/{down}"):
        inputs.resample_rule(rate)
    with pytest.raises(ValueError, match=f"{up}/{down}"):
        inputs.resample_audio(torch.zeros(100), rate)


def test_entry_points_are_declared_bound_and_exported_by_both_libraries():
    hdr = open(os.path.join(ROOT, "include", "csts_hip.h")).read()
    assert re.search(r"\bint\s+csts_resample_wav\s*\(", hdr) and re.search(r"\bint64_t\s+csts_resample_len\s*\(", hdr)
    for name, value in (("CSTS_RESAMPLE_RUN", lib.RESAMPLE_RUN), ("CSTS_RESAMPLE_MAX_LDS_FLOATS", lib.RESAMPLE_MAX_LDS_FLOATS)):
        assert int(re.search(rf"#define {name} (\d+)", hdr).group(1)) == value
    assert int(re.search(r"#define CSTS_ABI_VERSION (\d+)", hdr).group(1)) == lib.ABI_VERSION
    for path in lib._PATHS.values():
        so = ctypes.CDLL(path)
        assert hasattr(so, "csts_resample_wav") and hasattr(so, "csts_resample_len"), path
    handle = lib.load()
    assert "csts_resample_wav" in lib.SYMBOLS and "csts_resample_len" in lib.SYMBOLS and handle.csts_resample_wav
    code = ("from csts_amd import lib; lib.set_half('fp16'); h = lib.load(); assert h.csts_resample_len(147, 80, 147) == 80; "
            "assert h.csts_resample_wav(None, 0, 1, 1, 1, None, 1, 2, 20, None, None) != 0; print('ok')")
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.startswith("ok"), p.stderr[-2000:]


def test_bad_arguments_return_the_error_code_without_a_launch():
    """Every refusal happens on the host before the launch, so it shows on a machine without a GPU.  The pointers are host arrays:
    a call that passed the checks would hand them to a kernel, so every call here fails one."""
    handle = lib.load()
    x, taps, out = np.zeros(64, np.float32), np.zeros(41, np.float32), np.zeros(64, np.float32)
    px, pt, po = x.ctypes.data, taps.ctypes.data, out.ctypes.data

    def call(wav=px, kind=lib.WAV_F32, B=1, C=1, n=64, tp=pt, up=1, down=2, half=20, o=po):
        return handle.csts_resample_wav(wav, kind, B, C, n, tp, up, down, half, o, None)

    bad = [dict(wav=None), dict(tp=None), dict(o=None), dict(kind=2), dict(kind=-1), dict(B=0), dict(B=65536), dict(C=0), dict(C=65),
           dict(n=0), dict(n=-5), dict(n=(1 << 40) + 1), dict(up=0), dict(up=-1), dict(down=0), dict(half=0), dict(half=-20),
           dict(up=(1 << 20) + 1), dict(down=(1 << 20) + 1),
           dict(up=24000, down=24001, half=240010),            # the table does not fit
           dict(up=1, down=64, half=640)]                        # one run's input span does not fit
    for kw in bad:
        assert call(**kw) == -1, kw
        assert b"csts_resample_wav" in handle.csts_last_error(), kw
    assert inputs.resample_lds_floats(1, 64, 640) > lib.RESAMPLE_MAX_LDS_FLOATS
    for n, up, down in ((0, 1, 2), (-1, 1, 2), (10, 0, 2), (10, 1, 0), ((1 << 40) + 1, 1, 2), (10, (1 << 20) + 1, 1)):
        assert handle.csts_resample_len(n, up, down) == -1
    assert handle.csts_resample_len(1 << 40, 1 << 20, 1) == 1 << 60


def test_toy_dataset_writes_the_rate(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from make_toy_dataset import write_dataset
    plain, rated = str(tmp_path / "plain"), str(tmp_path / "rated")
    write_dataset(plain, clips_per_video=(1,), sizes=((8, 8),), test_clips=1, seed=3)
    write_dataset(rated, clips_per_video=(1,), sizes=((8, 8),), test_clips=1, seed=3, sample_rate=48000)
    name = os.path.join("clips", "video00", "video00_t0_t5.npz")
    with np.load(os.path.join(plain, name)) as a, np.load(os.path.join(rated, name)) as b:
        assert sorted(a.files) == ["fps", "frames_u8", "wav"] and a["wav"].shape == (24000 * 5,)
        assert sorted(b.files) == ["fps", "frames_u8", "sample_rate", "wav"] and b["wav"].shape == (48000 * 5,)
        assert int(b["sample_rate"]) == 48000 and np.array_equal(a["frames_u8"], b["frames_u8"])
