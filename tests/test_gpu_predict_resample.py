"""Audio at any sample rate, model level: GazePredictor.predict_video / predict with sample_rate, and ClipStore on clips that
carry a sample_rate entry.  The predictor of tests/test_gpu_predict_video.py: random weights, the Ego4D forecast YAML, fp32
compute, 200 frames of 64 x 80; the waveform is 48 kHz noise of the matching length (1600 samples a frame at 30 fps).

The module's fixture runs predict_video without a rate BEFORE its first resampling call and again after every other call: the
two must agree bit for bit.  Everything here is an identity between two paths through the same kernels, so every comparison is
torch.equal."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from csts_amd import GazePredictor  # noqa: E402
from csts_amd import datasets as D, inputs  # noqa: E402
from csts_amd.config import load_yaml  # noqa: E402
from make_toy_dataset import write_dataset  # noqa: E402

DEV = torch.device("cuda:0")
YAML = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml")
N, H, W, STRIDE, BATCH = 200, 64, 80, 32, 2
KEYS = ("points", "peak", "count", "heatmaps")


def same(a, b, keys=KEYS):
    return all(torch.equal(a[k].nan_to_num(-1.0), b[k].nan_to_num(-1.0)) for k in keys)


@pytest.fixture(scope="module")
def run():
    cfg = load_yaml(YAML, ["NUM_GPUS", 1, "CSTS_AMD.COMPUTE", "fp32"])
    torch.manual_seed(5)
    predictor = GazePredictor(cfg, device=DEV, graph=True)
    g = torch.Generator().manual_seed(21)
    frames = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8).to(DEV)
    wav24 = (0.1 * torch.randn(N * 24000 // 30, generator=g)).to(DEV)
    wav48 = (0.1 * torch.randn(2, N * 48000 // 30, generator=g)).to(DEV)
    before = predictor.predict_video(frames, wav24, stride=STRIDE, batch=BATCH)          # no resampling call has been made here
    return {"cfg": cfg, "predictor": predictor, "frames": frames, "wav24": wav24, "wav48": wav48, "before": before}


def test_rate_equals_resampling_first_and_differs_from_the_silent_error(run):
    predictor, frames, wav48 = run["predictor"], run["frames"], run["wav48"][0]
    got = predictor.predict_video(frames, wav48, stride=STRIDE, batch=BATCH, sample_rate=48000)
    pre = inputs.resample_audio(wav48, 48000)
    assert pre.shape == run["wav24"].shape
    want = predictor.predict_video(frames, pre, stride=STRIDE, batch=BATCH)
    assert set(got) == set(want) and got["windows"] == want["windows"] and int((got["count"] > 0).sum()) > 0
    assert same(got, want)
    wrong = predictor.predict_video(frames, wav48, stride=STRIDE, batch=BATCH)           # 48 kHz taken for 24 kHz
    assert not torch.equal(wrong["heatmaps"], got["heatmaps"])


def test_stereo_and_int16_with_a_rate(run):
    predictor, frames, stereo = run["predictor"], run["frames"], run["wav48"]
    got = predictor.predict_video(frames, stereo, stride=STRIDE, batch=BATCH, sample_rate=48000)
    want = predictor.predict_video(frames, inputs.resample_audio(stereo[None], 48000)[0], stride=STRIDE, batch=BATCH)
    assert same(got, want)
    pcm = (stereo * 32767.0).round().clamp(-32768, 32767).to(torch.int16)
    got = predictor.predict_video(frames, pcm, stride=STRIDE, batch=BATCH, sample_rate=np.int64(48000))
    want = predictor.predict_video(frames, inputs.resample_audio(pcm[None], 48000)[0], stride=STRIDE, batch=BATCH)
    assert same(got, want)
    with pytest.raises(ValueError):
        predictor.predict_video(frames, stereo, stride=STRIDE, batch=BATCH)             # 2-D without a rate
    for rate in (0, -1, 48000.0, "48000"):
        with pytest.raises(ValueError, match="positive integer"):
            predictor.predict_video(frames, stereo, stride=STRIDE, batch=BATCH, sample_rate=rate)


def test_predict_with_a_rate(run):
    predictor, frames = run["predictor"], run["frames"]
    T = run["cfg"].DATA.NUM_FRAMES
    clip = frames[:2 * T].reshape(2, T, H, W, 3)
    wav = 0.1 * torch.randn(2, 2, 44100 * 5, generator=torch.Generator().manual_seed(8)).to(DEV)
    idx = torch.linspace(10, 80, T, device=DEV)[None].repeat(2, 1)
    keys = ("points", "peak", "heatmaps", "rescaled")
    got = predictor.predict(clip, wav, idx, 150.0, sample_rate=44100)
    want = predictor.predict(clip, inputs.resample_audio(wav, 44100), idx, 150.0)
    assert same(got, want, keys)
    mono = predictor.predict(clip, wav[:, 0], idx, 150.0, sample_rate=44100)
    assert same(mono, predictor.predict(clip, inputs.resample_audio(wav[:, 0], 44100), idx, 150.0), keys)
    assert not torch.equal(mono["heatmaps"], got["heatmaps"])
    with pytest.raises(ValueError):
        predictor.predict(clip, wav, idx, 150.0)                                        # (B, C, n) without a rate
    with pytest.raises(ValueError, match="positive integer"):
        predictor.predict(clip, wav, idx, 150.0, sample_rate=44100.0)


S = 32
OPTS = ["NUM_GPUS", 1, "DATA.TRAIN_CROP_SIZE", S, "DATA.TEST_CROP_SIZE", S, "DATA.TRAIN_JITTER_SCALES", [32, 40],
        "CSTS_AMD.SYNTHETIC_DATA", False]


def test_clip_store_honours_the_rate_of_a_clip(tmp_path):
    rated, plain = str(tmp_path / "rated"), str(tmp_path / "plain")
    write_dataset(rated, clips_per_video=(2, 1), sizes=((36, 48), (40, 44)), test_clips=3, seed=1, sample_rate=48000)
    write_dataset(plain, clips_per_video=(2, 1), sizes=((36, 48), (40, 44)), test_clips=3, seed=1)
    for root, rate in ((rated, 48000), (plain, None)):
        store = D.ClipStore(load_yaml(YAML, OPTS + ["CSTS_AMD.DATA_ROOT", root]), "test", DEV)
        assert len(store) == 3
        store.upload()
        arena = store.spec_arena.cpu().numpy()
        for i, (video, name, _, _) in enumerate(store.clips):
            with np.load(os.path.join(root, "clips", video, name + ".npz")) as z:
                wav = torch.from_numpy(z["wav"]).to(DEV)
                assert ("sample_rate" in z.files) == (rate is not None)
            assert wav.shape == ((rate or 24000) * 5,)
            if rate is not None:
                wav = inputs.resample_audio(wav, rate)
                assert wav.shape == (24000 * 5,)
            want = inputs.stft_logpower(wav[None])[0].cpu().numpy()                     # without a rate: what the store did before
            assert store.spec_host[i].shape == want.shape and np.array_equal(store.spec_host[i], want)
            off, stride, usable = store.specs_host[i].tolist()
            assert (stride, usable) == (want.shape[1], 86 * want.shape[1] // 150)
            assert np.array_equal(arena[off:off + want.size], want.reshape(-1))


def test_no_rate_keeps_its_bits_after_resampling_calls(run):
    predictor, frames, wav24 = run["predictor"], run["frames"], run["wav24"]
    inputs.resample_audio(run["wav48"], 48000)                                           # at least one, whatever ran before
    again = predictor.predict_video(frames, wav24, stride=STRIDE, batch=BATCH)
    assert same(again, run["before"], KEYS + ("rescaled",))
    at_rate = predictor.predict_video(frames, wav24, stride=STRIDE, batch=BATCH, sample_rate=24000)    # the identity: no launch
    assert same(at_rate, run["before"], KEYS + ("rescaled",))
