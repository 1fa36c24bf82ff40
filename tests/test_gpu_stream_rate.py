"""GazeStream(input_rate=R): audio pushed at R Hz and resampled inside the stream with the filter state carried from push to push.
Each window equals, bit for bit, the composition clip_sample + stft_logpower(resample_audio(whole waveform, R)) + audio_windows_at
+ predict_batch at stream_window's indices -- for every chunking.  The set-up of tests/test_gpu_stream.py: random weights, bf16,
the Ego4D forecast YAML, 104 frames of 64 x 80, stride 9 (windows 0..2); the audio is 104 * 1600 samples at 48 kHz, of which
83 190 24-kHz samples are final before close and window 2 needs 83 040."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from csts_amd import GazePredictor, inputs, stream_schedule, stream_window  # noqa: E402
from csts_amd.config import load_yaml  # noqa: E402
from csts_amd.infer import _picture_hw  # noqa: E402

DEV = torch.device("cuda:0")
YAML = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml")
N, H, W, STRIDE, PER48, PER441 = 104, 64, 80, 9, 1600, 1470
KEYS = ("points", "peak", "heatmaps", "rescaled")


@pytest.fixture(scope="module")
def env():
    cfg = load_yaml(YAML, ["NUM_GPUS", 1, "CSTS_AMD.COMPUTE", "bf16"])
    torch.manual_seed(5)
    predictor = GazePredictor(cfg, device=DEV, graph=True)
    g = torch.Generator().manual_seed(33)
    frames = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8).to(DEV)
    wav48 = (0.1 * torch.randn(N * PER48, generator=g)).to(DEV)
    wav24 = inputs.resample_audio(wav48, 48000)
    e = {"cfg": cfg, "predictor": predictor, "frames": frames, "wav48": wav48, "wav24": wav24,
         "spec": inputs.stft_logpower(wav24[None])[0]}
    s = predictor.stream(stride=STRIDE, input_rate=48000)
    e["plan"] = s.plan
    e["once"] = s.push(frames, wav48)                             # everything in one push, batch 1
    e["once_stream"] = s
    return e


def compose(e, groups, frames=None, spec=None, slices=False):
    """The windows of `groups` (lists of window numbers, one predict_batch call each) from public pieces.  slices: cut the audio
    windows as spec[:, c - 128 : c + 128] (for centres audio_windows_at would clamp at the end of a spectrogram)."""
    predictor, plan = e["predictor"], e["plan"]
    frames = e["frames"] if frames is None else frames
    spec = e["spec"] if spec is None else spec
    Hh, Ww, _ = _picture_hw(frames, 1, "rgb24", "bt601", False)
    row = predictor._video_params_row(Hh, Ww)
    nb = max(len(g) for g in groups)
    out = {}
    for g in groups:
        wins = [stream_window(plan, w) for w in g]
        rows = wins + [wins[-1]] * (nb - len(wins))
        idx = torch.from_numpy(np.stack([r["frames_idx"] for r in rows]).astype(np.int32)).to(DEV)
        cen = torch.from_numpy(np.stack([r["audio_centers"] for r in rows]).astype(np.int32)).to(DEV)
        if slices:
            audio = torch.stack([torch.stack([spec[:, c - 128:c + 128] for c in r]) for r in cen.tolist()])[:, None]
        else:
            assert int(cen.min()) >= 128 and int(cen.max()) <= spec.shape[1] - 1 - 128   # audio_windows_at clamps nothing here
            audio = inputs.audio_windows_at(spec, cen)
        params = torch.tensor([row], dtype=torch.int32, device=DEV).repeat(nb, 1)
        video = inputs.clip_sample(frames, idx, params, 256, mean=tuple(e["cfg"].DATA.MEAN), std=tuple(e["cfg"].DATA.STD))
        res = predictor.predict_batch({"video": video, "audio": audio})
        for i, w in enumerate(g):
            out[w] = {k: res[k][i] for k in KEYS}
    return out


def same(results, want):
    assert [r["window"] for r in results] == sorted(want)
    for r in results:
        for k in KEYS:
            assert torch.equal(r[k], want[r["window"]][k]), (r["window"], k)


def test_one_push_equals_the_composition_on_the_resampled_waveform(env):
    res, s = env["once"], env["once_stream"]
    assert inputs.resample_ready(N * PER48, 1, 2, 20) == 83190 and stream_window(env["plan"], 2)["ready_samples"] == 83040
    assert [r["window"] for r in res] == [0, 1, 2] == stream_schedule(env["plan"], [(N, N * PER48)], input_rate=48000)[0]
    assert (s.frames, s.samples, s.input_samples, s.resampler.consumed, s.resampler.produced) == (N, 83190, N * PER48, N * PER48, 83190)
    same(res, compose(env, [[0], [1], [2]]))
    # a stream fed the plain decimation at 24 kHz sees another track
    naive = env["predictor"].stream(stride=STRIDE).push(env["frames"], env["wav48"][::2].contiguous())
    assert [r["window"] for r in naive] == [0, 1, 2]
    assert not any(torch.equal(a["heatmaps"], b["heatmaps"]) for a, b in zip(res, naive))


@pytest.mark.parametrize("name", ["one_frame_a_push", "ragged_audio_a_second_ahead"])
def test_chunking_does_not_change_a_bit(env, name):
    sizes = [1, 5, 11, 32, 2, 40, 13]
    assert sum(sizes) == N
    if name == "one_frame_a_push":
        pushes = [(1, PER48)] * N
    else:
        pushes, left = [(0, 30 * PER48)], (N - 30) * PER48
        for k in sizes:
            pushes.append((k, min(k * PER48, left)))
            left -= pushes[-1][1]
    assert sum(p[0] for p in pushes) == N and sum(p[1] for p in pushes) == N * PER48
    s = env["predictor"].stream(stride=STRIDE, input_rate=48000)
    fa = sa = 0
    per_push, flat = [], []
    for k, m in pushes:
        r = s.push(env["frames"][fa:fa + k] if k else None, env["wav48"][sa:sa + m] if m else None)
        fa, sa = fa + k, sa + m
        per_push.append([x["window"] for x in r])
        flat += r
        assert s.input_samples == sa == s.resampler.consumed and s.samples == s.resampler.produced
    assert per_push == stream_schedule(env["plan"], pushes, input_rate=48000)
    assert [r["window"] for r in flat] == [0, 1, 2]
    for r, ref in zip(flat, env["once"]):
        for k in KEYS:
            assert torch.equal(r[k], ref[k]), (name, r["window"], k)


def test_int16_stereo_at_44100_chunked(env):
    g = torch.Generator().manual_seed(36)
    pcm = torch.randint(-3000, 3000, (2, N * PER441), generator=g, dtype=torch.int16).to(DEV)
    wav24 = inputs.resample_audio(pcm[None], 44100)[0]
    spec = inputs.stft_logpower(wav24[None])[0]
    s = env["predictor"].stream(stride=STRIDE, input_rate=44100)
    flat, pushes = [], []
    for a in range(0, N, 8):
        b = min(a + 8, N)
        flat += s.push(env["frames"][a:b], pcm[:, a * PER441:b * PER441])
        pushes.append((b - a, (b - a) * PER441))
    assert (s.resampler.channels, s.resampler.dtype) == (2, torch.int16) and s.input_samples == N * PER441
    assert [r["window"] for r in flat] == [0, 1, 2] == [w for ws in stream_schedule(env["plan"], pushes, input_rate=44100) for w in ws]
    same(flat, compose(env, [[0], [1], [2]], spec=spec))


def test_audio_too_far_ahead_raises_and_consumes_nothing(env):
    s = env["predictor"].stream(stride=STRIDE, input_rate=48000)
    quiet = torch.zeros(2 * 120 * 832 + 100, device=DEV)          # 99 870 samples at 24 kHz: more than the ring's 832 columns
    assert s.resampler.count(quiet.numel()) > 120 * 832
    with pytest.raises(ValueError, match="832 columns"):
        s.push(None, quiet)
    assert (s.frames, s.samples, s.cols, s.input_samples, s.resampler.consumed, s.resampler.produced) == (0, 0, 0, 0, 0, 0)
    with pytest.raises(ValueError, match="fixed by the first push|must be"):
        s.push(None, quiet[:100].reshape(1, 1, 100))
    assert s.push(None, quiet[:2 * 120 * 831 + 20]) == [] and s.cols == 831 and s.samples == 120 * 831     # 20 inputs are held back


def test_close_flushes_the_resampler_before_the_last_column(env):
    cut48 = 137160                                                # 68 580 samples at 24 kHz, 68 570 of them final before close
    s = env["predictor"].stream(stride=STRIDE, input_rate=48000)
    assert s.push(env["frames"][:86], env["wav48"][:cut48]) == [] and s.cols == 571 and s.samples == 68570
    done = s.close()
    assert [r["window"] for r in done] == [0] and s.cols == 572 and s.samples == 68580 and s.dropped == 7
    wav24 = inputs.resample_audio(env["wav48"][:cut48], 48000)
    offline = inputs.stft_logpower(wav24[None])[0]
    assert wav24.numel() == 68580 and offline.shape[1] == 572
    same(done, compose(env, [[0]], spec=offline, slices=True))
    assert not torch.equal(done[0]["heatmaps"], env["once"][0]["heatmaps"])
    s = env["predictor"].stream(stride=STRIDE, input_rate=48000)
    assert s.push(env["frames"][:86], env["wav48"][:cut48]) == []
    assert s.close(wav_pad=False) == [] and s.dropped == 8 and s.samples == 68580
    with pytest.raises(ValueError, match="closed"):
        s.push(None, env["wav48"][:10])
