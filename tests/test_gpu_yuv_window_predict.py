"""GazePredictor on decoder surfaces: predict, predict_video(overlay=True) with the RGB and the nv12 overlay and
stream(...).push_live(..., overlay=True) on a padded nv12 recording (surfaces of 72 x 96 holding pictures of 64 x 80 at (4, 6))
equal, in every returned entry (torch.equal), the same call on inputs.yuv_window of it; 4:2:0 overlays are compared through
yuv_window and equal the input outside the window; points_source is normalised on the window's H x W; the groups refuse a
window.  120 frames, stride 16, batch 3, random weights, fp32."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from csts_amd import GazePredictor, GazeStreamGroup, inputs  # noqa: E402
from csts_amd.config import load_yaml  # noqa: E402
from csts_amd.infer import points_to_source  # noqa: E402

DEV = torch.device("cuda:0")
YAML = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml")
N, HS, WS, STRIDE, BATCH = 120, 72, 96, 16, 3
WINDOW = (4, 6, 64, 80)
H, W = WINDOW[2:]
FMT = dict(pixel_format="nv12", matrix="bt709", full_range=False)


def _same(a, b, skip=()):
    assert set(a) == set(b)
    for k in a:
        if k in skip:
            continue
        if torch.is_tensor(a[k]):
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
            assert torch.equal(a[k].nan_to_num(-1.0) if a[k].is_floating_point() else a[k],
                               b[k].nan_to_num(-1.0) if b[k].is_floating_point() else b[k]), k
        elif hasattr(a[k], "shape"):
            assert (a[k] == b[k]).all(), k
        else:
            assert a[k] == b[k], k


def _surface_overlay(got, want, surfaces):
    """A 4:2:0 overlay of surfaces: the tight overlay inside the window, the input outside it."""
    assert got.shape == surfaces.shape and got.dtype == torch.uint8
    assert torch.equal(inputs.yuv_window(got, "nv12", WINDOW), want)
    probe = torch.arange(HS * 3 // 2 * WS).view(1, HS * 3 // 2, WS)
    mask = torch.zeros(HS * 3 // 2 * WS, dtype=torch.bool)
    mask[inputs.yuv_window(probe, "nv12", WINDOW).reshape(-1)] = True
    mask = mask.view(HS * 3 // 2, WS).to(DEV)
    assert torch.equal(torch.where(mask, surfaces, got), surfaces)
    assert not torch.equal(got, surfaces)


@pytest.fixture(scope="module")
def run():
    cfg = load_yaml(YAML, ["NUM_GPUS", 1, "CSTS_AMD.COMPUTE", "fp32"])
    torch.manual_seed(5)
    predictor = GazePredictor(cfg, device=DEV, graph=True)
    g = torch.Generator().manual_seed(23)
    surf = torch.randint(0, 256, (N, HS * 3 // 2, WS), generator=g, dtype=torch.uint8).to(DEV)
    wav = (0.1 * torch.randn(N * 24000 // 30, generator=g)).to(DEV)
    return {"cfg": cfg, "predictor": predictor, "surf": surf, "tight": inputs.yuv_window(surf, "nv12", WINDOW), "wav": wav}


def test_predict(run):
    predictor, surf, tight = run["predictor"], run["surf"], run["tight"]
    T = int(run["cfg"].DATA.NUM_FRAMES)
    wav = run["wav"][None, :24000 * 3]
    idx = (torch.arange(T, dtype=torch.float32, device=DEV) + 0.5)[None]
    lab = torch.rand(1, T, 2, dtype=torch.float64, device=DEV)
    got = predictor.predict(surf[None, :T], wav, idx, float(T), labels=lab, attention=True, window=WINDOW, **FMT)
    want = predictor.predict(tight[None, :T], wav, idx, float(T), labels=lab, attention=True, **FMT)
    _same(got, want)
    # the attention maps drawn onto the surfaces: RGB of the window, and 4:2:0 inside the surfaces
    rgb = predictor.render_attention(surf[None, :T], got, points=got["points"], window=WINDOW, **FMT)
    assert rgb.shape == (1, T, H, W, 3)
    assert torch.equal(rgb, predictor.render_attention(tight[None, :T], want, points=want["points"], **FMT))
    yuv = predictor.render_attention(surf[None, :T], got, points=got["points"], out_format="nv12", window=WINDOW, **FMT)
    _surface_overlay(yuv[0], predictor.render_attention(tight[None, :T], want, points=want["points"], out_format="nv12", **FMT)[0],
                     surf[:T])
    with pytest.raises(ValueError, match="window"):
        predictor.predict(surf[None, :T], wav, idx, float(T), window=(4, 6, 64, 92), **FMT)
    with pytest.raises(ValueError, match="rgb24"):
        predictor.predict(torch.zeros(1, T, H, W, 3, dtype=torch.uint8, device=DEV), wav, idx, float(T), window=WINDOW)


def test_predict_video_and_overlays(run):
    predictor, surf, tight, wav = run["predictor"], run["surf"], run["tight"], run["wav"]
    kw = dict(stride=STRIDE, batch=BATCH, overlay=True, attention_track=True, fill="linear")
    got = predictor.predict_video(surf, wav, window=WINDOW, **kw, **FMT)
    want = predictor.predict_video(tight, wav, **kw, **FMT)
    _same(got, want)
    assert got["overlay"].shape == (N, H, W, 3) and got["windows"] == 3 and 0 < int((got["count"] > 0).sum()) < N
    # points_source is normalised on the window's H x W, not on the surface's
    row = predictor._video_params_row(H, W)
    S = int(run["cfg"].DATA.TEST_CROP_SIZE)
    assert torch.equal(got["points_source"].nan_to_num(-1.0), points_to_source(got["points"], row, S).nan_to_num(-1.0))
    assert row != predictor._video_params_row(HS, WS)
    # the overlay in the recording's own layout: the surfaces' shape, the tight overlay inside the window, the input around it
    got_yuv = predictor.predict_video(surf, wav, window=WINDOW, overlay_format="nv12", **kw, **FMT)
    want_yuv = predictor.predict_video(tight, wav, overlay_format="nv12", **kw, **FMT)
    _same(got_yuv, want_yuv, skip=("overlay",))
    _surface_overlay(got_yuv["overlay"], want_yuv["overlay"], surf)
    # the renderers on their own: chunked, in place, and the attention track
    for chunk in (None, 7):
        assert torch.equal(predictor.render_track(surf, got, chunk=chunk, window=WINDOW, **FMT), want["overlay"])
    buf = surf.clone()
    assert predictor.render_track(buf, got, chunk=33, out=buf, out_format="nv12", window=WINDOW, **FMT) is buf
    assert torch.equal(buf, got_yuv["overlay"])
    att = predictor.render_attention_track(surf, got, points=got["points"], chunk=50, window=WINDOW, **FMT)
    assert torch.equal(att, predictor.render_attention_track(tight, want, points=want["points"], chunk=50, **FMT))
    att = predictor.render_attention_track(surf, got, points=got["points"], out_format="nv12", window=WINDOW, **FMT)
    _surface_overlay(att, predictor.render_attention_track(tight, want, points=want["points"], out_format="nv12", **FMT), surf)
    with pytest.raises(ValueError, match="window"):
        predictor.predict_video(surf, wav, window=(5, 6, 64, 80), **FMT)


@pytest.mark.parametrize("overlay_format", [None, "nv12"])
def test_push_live(run, overlay_format):
    predictor, surf, tight, wav = run["predictor"], run["surf"], run["tight"], run["wav"]
    kw = dict(stride=STRIDE, batch=BATCH, live="linear", overlay=True, overlay_format=overlay_format, **FMT)
    a, b = predictor.stream(window=WINDOW, **kw), predictor.stream(**kw)
    per = wav.numel() // N
    f = 0
    for k in (7, 40, 1, 32, 40):                             # pieces of any size, one longer than max_chunk
        pa = a.push_live(surf[f:f + k], wav[f * per:(f + k) * per])
        pb = b.push_live(tight[f:f + k], wav[f * per:(f + k) * per])
        assert len(pa[0]) == len(pb[0])
        for ra, rb in zip(pa[0], pb[0]):
            _same(ra, rb)
        _same(pa[1], pb[1], skip=("overlay",) if overlay_format else ())
        if overlay_format:
            assert pa[1]["overlay"].shape == (k, HS * 3 // 2, WS)
            assert torch.equal(inputs.yuv_window(pa[1]["overlay"], "nv12", WINDOW), pb[1]["overlay"])
        else:
            assert pa[1]["overlay"].shape == (k, H, W, 3)
        f += k
    assert a.hw == b.hw == (H, W) and a.next_window == b.next_window > 0
    empty = a.push_live(None, None)[1]["overlay"]
    assert tuple(empty.shape) == ((0, HS * 3 // 2, WS) if overlay_format else (0, H, W, 3))
    for x, y in zip(a.close(), b.close()):
        _same(x, y)


def test_the_groups_refuse_a_window(run):
    predictor = run["predictor"]
    with pytest.raises(ValueError, match="window"):
        GazeStreamGroup(predictor, 2, window=WINDOW, **FMT)
    with pytest.raises(ValueError, match="window"):
        predictor.stream_group(2, window=WINDOW, **FMT)
    with pytest.raises(ValueError, match="window"):
        predictor.live_group(2, "linear", window=WINDOW, **FMT)
    with pytest.raises(ValueError, match="rgb24"):
        predictor.stream(window=WINDOW)
    with pytest.raises(ValueError, match="odd"):
        predictor.stream(window=(1, 0, 64, 80), **FMT)
