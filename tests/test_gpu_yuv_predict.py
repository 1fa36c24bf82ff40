"""GazePredictor on 4:2:0 recordings: predict, predict_video (with overlay=True) and render_track on an nv12 recording equal, in
every returned tensor (torch.equal), the same calls on inputs.yuv_to_rgb of it; out= aliasing the 4:2:0 input is refused.  120
frames of 64 x 80, stride 16, batch 3, random weights, fp32; the chunked renderers (render_track, render_attention_track) also on
50 x 70 pictures, whose chunks start at no multiple of 16 bytes."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from csts_amd import GazePredictor, inputs  # noqa: E402
from csts_amd.config import load_yaml  # noqa: E402

DEV = torch.device("cuda:0")
YAML = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml")
N, H, W, STRIDE, BATCH = 120, 64, 80, 16, 3
FMT = dict(pixel_format="nv12", matrix="bt709", full_range=False)


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        if torch.is_tensor(a[k]):
            assert a[k].dtype == b[k].dtype and torch.equal(a[k].nan_to_num(-1.0) if a[k].is_floating_point() else a[k],
                                                            b[k].nan_to_num(-1.0) if b[k].is_floating_point() else b[k]), k
        else:
            assert a[k] == b[k], k


@pytest.fixture(scope="module")
def run():
    cfg = load_yaml(YAML, ["NUM_GPUS", 1, "CSTS_AMD.COMPUTE", "fp32"])
    torch.manual_seed(5)
    predictor = GazePredictor(cfg, device=DEV, graph=True)
    g = torch.Generator().manual_seed(21)
    yuv = torch.randint(0, 256, (N, H * 3 // 2, W), generator=g, dtype=torch.uint8).to(DEV)
    wav = (0.1 * torch.randn(N * 24000 // 30, generator=g)).to(DEV)
    rgb = inputs.yuv_to_rgb(yuv, **FMT)
    return {"cfg": cfg, "predictor": predictor, "yuv": yuv, "rgb": rgb, "wav": wav}


def test_predict_video_and_overlay_equal_the_rgb_recording(run):
    predictor, yuv, rgb, wav = run["predictor"], run["yuv"], run["rgb"], run["wav"]
    got = predictor.predict_video(yuv, wav, stride=STRIDE, batch=BATCH, overlay=True, **FMT)
    want = predictor.predict_video(rgb, wav, stride=STRIDE, batch=BATCH, overlay=True)
    _same(got, want)
    assert got["overlay"].shape == (N, H, W, 3) and got["overlay"].dtype == torch.uint8 and got["windows"] == 3
    assert 0 < int((got["count"] > 0).sum()) < N
    # render_track: the whole, in chunks, and into a given output
    for chunk in (None, 7, 64):
        assert torch.equal(predictor.render_track(yuv, got, chunk=chunk, **FMT), want["overlay"]), chunk
    out = torch.empty(N, H, W, 3, dtype=torch.uint8, device=DEV)
    assert predictor.render_track(yuv, got, out=out, chunk=33, **FMT) is out and torch.equal(out, want["overlay"])
    # out aliasing the 4:2:0 input: by shape, and by memory
    with pytest.raises(ValueError):
        predictor.render_track(yuv, got, out=yuv, **FMT)
    whole = torch.zeros(N * H * W * 3, dtype=torch.uint8, device=DEV)
    inside = whole[:yuv.numel()].view_as(yuv).copy_(yuv)
    with pytest.raises(ValueError, match="share memory"):
        predictor.render_track(inside, got, out=whole.view(N, H, W, 3), **FMT)
    # a shape of the other kind is refused either way
    with pytest.raises(ValueError):
        predictor.predict_video(yuv, wav, stride=STRIDE, batch=BATCH)
    with pytest.raises(ValueError):
        predictor.predict_video(rgb, wav, stride=STRIDE, batch=BATCH, **FMT)
    with pytest.raises(ValueError, match="pixel_format"):
        predictor.predict_video(yuv, wav, pixel_format="yuyv")


def test_chunked_renderers_on_pictures_of_no_multiple_of_16_bytes(run):
    """50 x 70 pictures are 10500 bytes in RGB: with chunk=7 the second chunk of the output starts at byte 73500 (= 12 mod 16).
    render_track and render_attention_track convert chunk by chunk into those slices and equal the RGB recording's result."""
    predictor, wav = run["predictor"], run["wav"]
    h, w = 50, 70
    g = torch.Generator().manual_seed(23)
    yuv = torch.randint(0, 256, (N, h * 3 // 2, w), generator=g, dtype=torch.uint8).to(DEV)
    rgb = inputs.yuv_to_rgb(yuv, **FMT)
    kw = dict(stride=STRIDE, batch=BATCH, overlay=True, attention_track=True, fill="hold")
    got = predictor.predict_video(yuv, wav, **kw, **FMT)
    want = predictor.predict_video(rgb, wav, **kw)
    _same(got, want)
    assert got["overlay"].shape == (N, h, w, 3) and not torch.equal(got["overlay"], rgb)
    for chunk in (7, 1, 50, None):
        assert torch.equal(predictor.render_track(yuv, got, chunk=chunk, **FMT), want["overlay"]), chunk
    for head in (None, 0):
        ref = predictor.render_attention_track(rgb, want, head=head, points=want["points"])
        assert not torch.equal(ref, rgb)
        for chunk in (7, 33, None):
            drawn = predictor.render_attention_track(yuv, got, head=head, points=got["points"], chunk=chunk, **FMT)
            assert drawn.shape == (N, h, w, 3) and torch.equal(drawn, ref), (head, chunk)
    out = torch.empty(N, h, w, 3, dtype=torch.uint8, device=DEV)
    assert predictor.render_attention_track(yuv, got, out=out, chunk=7, **FMT) is out
    assert torch.equal(out, predictor.render_attention_track(rgb, want))
    with pytest.raises(ValueError):
        predictor.render_attention_track(yuv, got, out=yuv, **FMT)


def test_predict_equals_the_rgb_clip(run):
    predictor, yuv, rgb, wav = run["predictor"], run["yuv"], run["rgb"], run["wav"]
    T = int(run["cfg"].DATA.NUM_FRAMES)
    pick = torch.arange(0, 2 * T * 5, 5, device=DEV).view(2, T)
    clips_yuv, clips_rgb = yuv[pick], rgb[pick]                               # (2, T, 96, 80) and (2, T, 64, 80, 3)
    w = wav[:2 * 48000].view(2, 48000)
    fidx = (torch.arange(T, device=DEV, dtype=torch.float32) * 5)[None].expand(2, T).contiguous()
    g = torch.Generator().manual_seed(4)
    labels = torch.rand(2, T, 3, generator=g, dtype=torch.float64).to(DEV)
    got = predictor.predict(clips_yuv, w, fidx, 60.0, labels=labels, attention=True, **FMT)
    want = predictor.predict(clips_rgb, w, fidx, 60.0, labels=labels, attention=True)
    _same(got, want)
    drawn = predictor.render_attention(clips_yuv, got, points=got["points"], **FMT)
    assert drawn.shape == clips_rgb.shape and torch.equal(drawn, predictor.render_attention(clips_rgb, want, points=want["points"]))
    with pytest.raises(ValueError):
        predictor.render_attention(clips_yuv, got, out=clips_yuv, **FMT)


def test_frames_at_the_crop_size_take_the_identity_crop(run):
    predictor, wav = run["predictor"], run["wav"]
    S, T = int(run["cfg"].DATA.TEST_CROP_SIZE), int(run["cfg"].DATA.NUM_FRAMES)
    g = torch.Generator().manual_seed(6)
    clip = torch.randint(0, 256, (BATCH, T, S * 3 // 2, S), generator=g, dtype=torch.uint8).to(DEV)   # the graph shape of the video
    fidx = (torch.arange(T, device=DEV, dtype=torch.float32) * 5)[None].expand(BATCH, T).contiguous()
    w = wav[:BATCH * 32000].view(BATCH, 32000)
    got = predictor.predict(clip, w, fidx, 60.0, **FMT)
    want = predictor.predict(inputs.yuv_to_rgb(clip, **FMT), w, fidx, 60.0)
    _same(got, want)
