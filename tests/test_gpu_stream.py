"""GazeStream against the composition of public pieces: per window clip_sample of the whole video at stream_window's frames,
stft_logpower of the whole waveform + audio_windows_at at its centres, predict_batch at the same batch size -- bit for bit.
Random weights, bf16, the Ego4D forecast YAML; 104 frames of 64 x 80 with 83 200 samples, stride 9: windows 0..2, which share 7 of
their 8 input frames with their neighbour."""
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

from csts_amd import GazePredictor, inputs, ops, stream_schedule, stream_window, track_from_windows  # noqa: E402
from csts_amd.config import load_yaml  # noqa: E402
from csts_amd.infer import _picture_hw  # noqa: E402
from csts_amd.stream import ring_sizes  # noqa: E402

DEV = torch.device("cuda:0")
YAML = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml")
N, H, W, STRIDE, PER = 104, 64, 80, 9, 800
KEYS = ("points", "peak", "heatmaps", "rescaled")


@pytest.fixture(scope="module")
def env():
    cfg = load_yaml(YAML, ["NUM_GPUS", 1, "CSTS_AMD.COMPUTE", "bf16"])
    torch.manual_seed(5)
    predictor = GazePredictor(cfg, device=DEV, graph=True)
    g = torch.Generator().manual_seed(33)
    frames = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8).to(DEV)
    wav = (0.1 * torch.randn(N * PER, generator=g)).to(DEV)
    e = {"cfg": cfg, "predictor": predictor, "frames": frames, "wav": wav, "spec": inputs.stft_logpower(wav[None])[0]}
    s = predictor.stream(stride=STRIDE)
    e["plan"] = s.plan
    e["once"] = s.push(frames, wav)                               # everything in one push, batch 1
    return e


def compose(e, groups, frames=None, spec=None, slices=False, **fmt):
    """The windows of `groups` (lists of window numbers, one predict_batch call each, padded to the longest by repeating the last
    window) from public pieces.  slices: cut the audio windows as spec[:, c - 128 : c + 128] (for centres audio_windows_at would
    clamp at the end of a spectrogram)."""
    predictor, plan = e["predictor"], e["plan"]
    frames = e["frames"] if frames is None else frames
    spec = e["spec"] if spec is None else spec
    Hh, Ww, _ = _picture_hw(frames, 1, fmt.get("pixel_format", "rgb24"), fmt.get("matrix", "bt601"), fmt.get("full_range", False))
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
        video = inputs.clip_sample(frames, idx, params, 256, mean=tuple(e["cfg"].DATA.MEAN), std=tuple(e["cfg"].DATA.STD), **fmt)
        res = predictor.predict_batch({"video": video, "audio": audio})
        for i, w in enumerate(g):
            out[w] = {k: res[k][i] for k in KEYS}
    return out


def same(results, want):
    assert [r["window"] for r in results] == sorted(want)
    for r in results:
        for k in KEYS:
            assert torch.equal(r[k], want[r["window"]][k]), (r["window"], k)


def test_pushed_all_at_once_equals_the_composition(env):
    res = env["once"]
    assert [r["window"] for r in res] == [0, 1, 2] == stream_schedule(env["plan"], [(N, N * PER)])[0]
    for r in res:
        win = stream_window(env["plan"], r["window"])
        assert r["frames_idx"].tolist() == win["frames_idx"].tolist() and r["target_idx"].tolist() == win["target_idx"].tolist()
        assert r["points"].shape == (8, 2) and r["peak"].shape == (8,) and r["heatmaps"].shape == (8, 64, 64) == r["rescaled"].shape
    same(res, compose(env, [[0], [1], [2]]))
    assert not torch.equal(res[0]["heatmaps"], res[1]["heatmaps"])


def _run(env, pushes, **kw):
    """Push (frames, samples) counts in order; returns the per-push window numbers and the flat results."""
    s = env["predictor"].stream(stride=STRIDE, **kw)
    fa = sa = 0
    per_push, flat = [], []
    for k, m in pushes:
        r = s.push(env["frames"][fa:fa + k] if k else None, env["wav"][sa:sa + m] if m else None)
        fa, sa = fa + k, sa + m
        per_push.append([x["window"] for x in r])
        flat += r
    assert fa == N and sa == N * PER
    return per_push, flat, s


@pytest.mark.parametrize("name", ["one_frame_a_push", "ragged_audio_a_second_ahead", "audio_a_second_behind"])
def test_chunking_does_not_change_a_bit(env, name):
    sizes = [1, 5, 11, 32, 2, 40, 13]
    assert sum(sizes) == N
    if name == "one_frame_a_push":
        pushes = [(1, PER)] * N
    elif name == "ragged_audio_a_second_ahead":
        pushes, left = [(0, 30 * PER)], (N - 30) * PER
        for k in sizes:
            pushes.append((k, min(k * PER, left)))
            left -= pushes[-1][1]
    else:
        pushes = [(30, 0), (17, 17 * PER), (33, 33 * PER), (24, 24 * PER), (0, 30 * PER)]
    assert sum(p[0] for p in pushes) == N and sum(p[1] for p in pushes) == N * PER
    per_push, flat, _ = _run(env, pushes)
    assert per_push == stream_schedule(env["plan"], pushes)
    assert [r["window"] for r in flat] == [0, 1, 2]
    for r, ref in zip(flat, env["once"]):
        for k in KEYS:
            assert torch.equal(r[k], ref[k]), (name, r["window"], k)


def test_batch_2_equals_the_composition_with_the_same_grouping(env):
    s = env["predictor"].stream(stride=STRIDE, batch=2)
    res = s.push(env["frames"], env["wav"])
    # the push is worked off in sub-chunks of max_chunk = 32 frames: windows 0 and 1 are ready after 96 frames, window 2 after 104
    steps = [ws for _, _, ws in env["predictor"].stream(stride=STRIDE, batch=2)._steps(N, N * PER) if ws]
    assert steps == [[0, 1], [2]] == [ws for ws in stream_schedule(env["plan"], [(32, N * PER), (32, 0), (32, 0), (8, 0)]) if ws]
    want = compose(env, [[0, 1], [2]])                             # [2] is padded by repeating window 2
    same(res, want)


def test_long_push_with_default_rings(env):
    g = torch.Generator().manual_seed(34)
    n = 400
    frames = torch.randint(0, 256, (n, H, W, 3), generator=g, dtype=torch.uint8).to(DEV)
    wav = (0.1 * torch.randn(n * PER, generator=g)).to(DEV)
    s = env["predictor"].stream()                                  # default stride 64, default rings
    assert s.max_chunk == 32 and s.capacity == ring_sizes(s.plan, 32, 256)
    assert (s.capacity["slots"], s.capacity["ring_cols"]) == (86 + 32, 832)
    assert s.capacity["crop_bytes"] == 118 * 3 * 256 * 256 * 4 and s.capacity["spec_bytes"] == 256 * 832 * 4
    res = []
    pushes = [(40, 40 * PER)] * 10
    for i in range(10):
        res.append(s.push(frames[40 * i:40 * i + 40], wav[40 * PER * i:40 * PER * (i + 1)]))
    assert [[r["window"] for r in rs] for rs in res] == stream_schedule(s.plan, pushes)
    flat = [r for rs in res for r in rs]
    assert [r["window"] for r in flat] == [0, 1, 2, 3, 4]          # 86 + 64 w <= 400
    assert tuple(s._crops.shape) == (118, 3, 256, 256) and tuple(s._spec.shape) == (256, 832) and s._tail.numel() < 240
    e = dict(env, plan=s.plan)
    want = compose(e, [[4]], frames=frames, spec=inputs.stft_logpower(wav[None])[0])
    same(flat[-1:], want)


def test_audio_too_far_ahead_raises_and_consumes_nothing(env):
    s = env["predictor"].stream(stride=STRIDE)
    quiet = torch.zeros(120 * 832, device=DEV)
    with pytest.raises(ValueError, match="832 columns"):
        s.push(None, quiet)
    assert (s.frames, s.samples, s.cols) == (0, 0, 0)
    assert s.push(None, quiet[:120 * 831]) == [] and s.cols == 831
    with pytest.raises(ValueError, match="832 columns"):
        s.push(None, quiet[:120])
    assert s.push(env["frames"][:1]) == []
    with pytest.raises(ValueError, match="fixed by the first push"):
        s.push(env["frames"][:1, :32])


def test_nv12_streams_to_the_bits_of_the_converted_pictures(env):
    g = torch.Generator().manual_seed(35)
    yuv = torch.randint(0, 256, (N, H * 3 // 2, W), generator=g, dtype=torch.uint8).to(DEV)
    fmt = {"pixel_format": "nv12", "matrix": "bt709", "full_range": False}
    rgb = inputs.yuv_to_rgb(yuv, **fmt)
    a = env["predictor"].stream(stride=STRIDE, **fmt).push(yuv, env["wav"])
    b = env["predictor"].stream(stride=STRIDE).push(rgb, env["wav"])
    assert [r["window"] for r in a] == [0, 1, 2] == [r["window"] for r in b]
    for x, y in zip(a, b):
        for k in KEYS:
            assert torch.equal(x[k], y[k]), (x["window"], k)
    same(a, compose(env, [[0], [1], [2]], frames=yuv, **fmt))
    assert not torch.equal(a[0]["heatmaps"], env["once"][0]["heatmaps"])


def test_track_from_windows_equals_gaze_track(env):
    res = env["once"]
    track = track_from_windows(res, N + 60)
    preds = torch.cat([r["heatmaps"] for r in res])
    target = torch.from_numpy(np.concatenate([r["target_idx"] for r in res])).to(DEV)
    want = ops.gaze_track(preds, target, N + 60)
    assert track["windows"] == 3 and int(want["count"].sum()) > 0
    for k in ("points", "peak", "count", "heatmaps", "rescaled"):         # unpredicted frames carry NaN points
        assert torch.equal(torch.isnan(track[k]), torch.isnan(want[k])), k
        assert torch.equal(torch.nan_to_num(track[k].double(), nan=-1.0), torch.nan_to_num(want[k].double(), nan=-1.0)), k
    small = track_from_windows(res[:1], N, want=("points", "count"))
    assert sorted(small) == ["count", "points", "windows"]


def test_close_on_a_short_video_reports_the_dropped_windows(env):
    s = env["predictor"].stream(stride=STRIDE)
    assert [r["window"] for r in s.push(env["frames"][:90], env["wav"])] == [0]
    # frames 0..89 were pushed: windows 1..7 began (their first input 9 w + 22 < 90) and miss frames
    assert s.close() == [] and s.dropped == 7 and s.closed
    with pytest.raises(ValueError, match="closed"):
        s.push(env["frames"][90:])
    # the column close() adds completes a window: window 0 reads up to column 571, i.e. 572 columns; the running stream has 571
    # after 68 580 samples and the offline STFT of those samples has the 572nd, computed with zeros past the last sample
    cut = 68640 - 60
    s = env["predictor"].stream(stride=STRIDE)
    assert s.push(env["frames"][:86], env["wav"][:cut]) == [] and s.cols == 571
    done = s.close()
    assert [r["window"] for r in done] == [0] and s.cols == 572 and s.dropped == 7
    offline = inputs.stft_logpower(env["wav"][None, :cut])[0]
    assert offline.shape[1] == 572
    same(done, compose(env, [[0]], spec=offline, slices=True))
    assert not torch.equal(done[0]["heatmaps"], env["once"][0]["heatmaps"])
    s = env["predictor"].stream(stride=STRIDE)
    assert s.push(env["frames"][:86], env["wav"][:cut]) == []
    assert s.close(wav_pad=False) == [] and s.dropped == 8
