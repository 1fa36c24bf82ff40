"""Resampling on a live stream, the host side (no GPU): the progress rule (resample_ready, resample_first_input,
resample_inputs_for) against brute force and against its C twins, StreamResampler.count over a random cut, stream_schedule with
an input rate, the constructor's refusals, and the C-ABI declarations."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_reference as R  # noqa: E402

EGO4D = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml")
RATES = R.RATES + (24000,)
N_IN = tuple(range(400)) + (4099, 20011)
ENTRY_POINTS = ("csts_resample_stream", "csts_resample_ready", "csts_resample_first_input")


class _NoPredictor:
    """What GazeStream reads of a predictor before the first push: its configuration."""
    def __init__(self, cfg):
        self.cfg = cfg


def _cfg():
    from csts_amd import load_yaml
    return load_yaml(EGO4D, ["NUM_GPUS", 0])


def _brute_ready(n_in, up, down, half):
    """The number of outputs m whose last input floor((m down + half) / up) is among the first n_in."""
    m = 0
    while (m * down + half) // up <= n_in - 1:
        m += 1
    return m


@pytest.mark.parametrize("rate", RATES)
def test_progress_rule_against_brute_force_and_the_c_twins(rate):
    from csts_amd import inputs, lib
    h = lib.load()
    _, up, down, half = inputs.resample_rule(rate)
    assert (up, down) == R.ratio(rate)
    held = []
    for n_in in N_IN:
        ready = inputs.resample_ready(n_in, up, down, half)
        assert ready == _brute_ready(n_in, up, down, half), n_in
        assert inputs.resample_ready(n_in, up, down, half, closed=True) == R.out_len(n_in, up, down)
        assert h.csts_resample_ready(n_in, up, down, half, 0) == ready
        assert h.csts_resample_ready(n_in, up, down, half, 1) == R.out_len(n_in, up, down)
        first = inputs.resample_first_input(ready, up, down, half)
        assert first == max(-(-(ready * down - half) // up), 0) == h.csts_resample_first_input(ready, up, down, half)
        assert h.csts_resample_first_input(n_in, up, down, half) == inputs.resample_first_input(n_in, up, down, half)
        assert 0 <= n_in - first <= 2 * half // up + 2, n_in                     # the tail a stream keeps
        if ready:
            held.append(R.out_len(n_in, up, down) - ready)
    assert 10 <= min(held) and max(held) <= 30                                   # what an open stream holds back


@pytest.mark.parametrize("rate", RATES)
def test_inputs_for_is_the_exact_inverse(rate):
    from csts_amd import inputs
    _, up, down, half = inputs.resample_rule(rate)
    assert inputs.resample_inputs_for(0, up, down, half) == inputs.resample_inputs_for(-3, up, down, half) == 0
    for m_out in list(range(1, 400)) + [4099, 20011]:
        n_in = inputs.resample_inputs_for(m_out, up, down, half)
        assert n_in == ((m_out - 1) * down + half) // up + 1
        assert inputs.resample_ready(n_in, up, down, half) >= m_out > inputs.resample_ready(n_in - 1, up, down, half)


def test_the_c_twins_refuse_what_is_outside_the_limits():
    from csts_amd import lib
    h = lib.load()
    assert h.csts_resample_ready(-1, 1, 2, 20, 0) == -1 and h.csts_resample_ready((1 << 40) + 1, 1, 2, 20, 0) == -1
    assert h.csts_resample_ready(10, 0, 2, 20, 0) == -1 and h.csts_resample_ready(10, 1, 2, 0, 1) == -1
    assert h.csts_resample_first_input(-1, 1, 2, 20) == -1 and h.csts_resample_first_input(5, 1, (1 << 20) + 1, 20) == -1
    assert h.csts_resample_ready(1 << 40, 1 << 20, 1, 1 << 20, 1) == 1 << 60


@pytest.mark.parametrize("rate", (48000, 44100, 8000, 192000))
def test_count_over_a_random_cut_sums_to_ready(rate):
    from csts_amd import inputs
    rng = np.random.default_rng(rate)
    pieces = rng.integers(0, 3000, 40).tolist() + [0, 1]
    r = inputs.StreamResampler(rate)
    assert (r.up, r.down, r.half) == inputs.resample_rule(rate)[1:] and (r.consumed, r.produced, r.closed) == (0, 0, False)
    assert r.channels is None and r.dtype is None
    total = produced = 0
    for m in pieces:                                              # count() changes nothing: replay the bookkeeping by hand
        r.consumed, r.produced = total, produced
        c = r.count(m)
        assert c == inputs.resample_ready(total + m, r.up, r.down, r.half) - produced >= 0
        assert (r.consumed, r.produced) == (total, produced)
        total, produced = total + m, produced + c
    assert produced == inputs.resample_ready(sum(pieces), r.up, r.down, r.half)
    with pytest.raises(ValueError):
        r.count(-1)


def test_schedule_with_an_input_rate_converts_by_differences_of_ready():
    from csts_amd import inputs, plan_stream, stream_schedule
    plan = plan_stream(_cfg(), stride=9)
    _, up, down, half = inputs.resample_rule(48000)
    rng = np.random.default_rng(4)
    cuts = sorted(rng.choice(np.arange(1, 104), 12, replace=False).tolist())
    sizes = np.diff([0] + cuts + [104]).tolist()
    for pushes in ([(1, 1600)] * 104, [(0, 30 * 1600)] + [(k, k * 1600) for k in sizes], [(104, 104 * 1600)]):
        total, converted = 0, []
        for k, m in pushes:
            converted.append((k, inputs.resample_ready(total + m, up, down, half) - inputs.resample_ready(total, up, down, half)))
            total += m
        got = stream_schedule(plan, pushes, input_rate=48000)
        assert got == stream_schedule(plan, converted)
        assert sum(m for _, m in converted) == inputs.resample_ready(total, up, down, half)
    # 104 frames of 48 kHz audio: 83 190 samples are final before close, window 2 needs 83 040 of them
    assert inputs.resample_ready(104 * 1600, up, down, half) == 83190
    assert stream_schedule(plan, [(104, 104 * 1600)], input_rate=48000) == [[0, 1, 2]]
    assert stream_schedule(plan, [(104, 83200)]) == stream_schedule(plan, [(104, 83200)], input_rate=None) == [[0, 1, 2]]
    assert stream_schedule(plan, [(104, 83200)], input_rate=24000) == [[0, 1, 2]]   # mono fp32 at 24 kHz passes through
    with pytest.raises(ValueError):
        stream_schedule(plan, [(1, 800)], input_rate=24000.0)


def test_constructor_refusals():
    from csts_amd import GazeStream
    cfg = _cfg()
    for bad in (0, True, 24000.0, -48000, "48000"):
        with pytest.raises(ValueError, match="input_rate"):
            GazeStream(_NoPredictor(cfg), input_rate=bad)
    with pytest.raises(ValueError, match="one of them"):
        GazeStream(_NoPredictor(cfg), sample_rate=24000, input_rate=48000)
    with pytest.raises(ValueError, match="input_rate="):               # the old refusal now points at the new keyword
        GazeStream(_NoPredictor(cfg), sample_rate=48000)
    s = GazeStream(_NoPredictor(cfg), stride=9, input_rate=48000)
    assert s.input_rate == 48000 and (s.resampler.up, s.resampler.down, s.resampler.half) == (1, 2, 20)
    assert (s.samples, s.input_samples) == (0, 0)
    plain = GazeStream(_NoPredictor(cfg), stride=9)
    assert plain.input_rate is None and plain.resampler is None and plain.input_samples == 0


def test_header_declares_and_both_libraries_export_the_entry_points():
    from csts_amd import lib
    hdr = open(os.path.join(ROOT, "include", "csts_hip.h")).read()
    assert re.search(r"\bint\s+csts_resample_stream\s*\(", hdr)
    assert re.search(r"\bint64_t\s+csts_resample_ready\s*\(", hdr) and re.search(r"\bint64_t\s+csts_resample_first_input\s*\(", hdr)
    for name in ENTRY_POINTS:
        assert name in lib.SYMBOLS, name
        for kind in ("bf16", "fp16"):
            assert hasattr(ctypes.CDLL(lib._PATHS[kind]), name), (kind, name)
    h = lib.load()
    fake = ctypes.c_void_p(4096)
    assert h.csts_resample_stream(None, 0, 1, 0, 0, -1, None, 1, 2, 20, 5, 5, None, None) == 0        # m0 == m1: nothing to do
    assert h.csts_resample_stream(fake, 0, 1, 100, 0, -1, fake, 1, 2, 20, 0, 41, fake, None) == -1    # output 40 reads sample 100
    assert b"csts_resample_stream" in h.csts_last_error()
    assert h.csts_resample_stream(fake, 2, 1, 100, 0, -1, fake, 1, 2, 20, 0, 40, fake, None) == -1    # in_kind
    assert h.csts_resample_stream(fake, 0, 65, 100, 0, -1, fake, 1, 2, 20, 0, 40, fake, None) == -1   # C <= 64
    assert h.csts_resample_stream(fake, 0, 1, 100, 0, -1, fake, 1, 2, 20, 7, 5, fake, None) == -1     # m0 > m1
