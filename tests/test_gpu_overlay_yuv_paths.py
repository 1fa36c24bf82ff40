"""The 4:2:0 overlay through every layer that draws: GazePredictor.render_track / render_attention / render_attention_track with
out_format, predict_video(overlay_format=...), GazeStream and GazeLiveGroup with overlay_format.  Each result equals, byte for
byte, the `where` composition (tests/rgb_yuv_reference.py::compose) of the RGB-output result of the same call: D is that RGB
result, M the same renderer drawn with alpha = 1 over all-black RGB frames ("any channel non-zero"), out = where(M, rgb_to_yuv(D),
frames).  Every other entry of a result keeps the bits it has without the keyword.  104 frames of 64 x 80 (and 48 x 64 for the
second slot of the group), stride 9, random weights, the configuration of tests/test_gpu_stream_live.py."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

import rgb_yuv_reference as Q  # noqa: E402
from csts_amd import GazePredictor, inputs  # noqa: E402
from csts_amd.config import load_yaml  # noqa: E402

DEV = torch.device("cuda:0")
YAML = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml")
N, H, W, STRIDE, PER, BATCH = 104, 64, 80, 9, 800, 3
SHAPES = [(104, 64, 80), (104, 48, 64)]


def fmt_of(layout):
    return {"pixel_format": layout, "matrix": "bt709", "full_range": False}


def bits(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float32:
        return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    if a.dtype == torch.float64:
        return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))
    return torch.equal(a, b)


def same_but_overlay(a, b):
    assert set(a) == set(b)
    for k in a:
        if k == "overlay":
            continue
        if torch.is_tensor(a[k]):
            assert bits(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


def composed(frames, D, black, layout):
    """where(M, rgb_to_yuv(D), frames) on the host -> uint8 like frames, and M; frames (n, h * 3 / 2, w), D and black (n, h, w, 3)."""
    M = (black.cpu().numpy() != 0).any(axis=-1)
    fmt = fmt_of(layout)
    want, _ = Q.compose(frames.cpu().numpy(), D.cpu().numpy(), M, layout, fmt["matrix"], fmt["full_range"])
    return want, M


def black_like(n, h, w):
    return torch.zeros(n, h, w, 3, dtype=torch.uint8, device=DEV)


@pytest.fixture(scope="module")
def env():
    cfg = load_yaml(YAML, ["NUM_GPUS", 1, "CSTS_AMD.COMPUTE", "bf16"])
    torch.manual_seed(5)
    predictor = GazePredictor(cfg, device=DEV, graph=True)
    recs = []
    for i, (n, h, w) in enumerate(SHAPES):
        g = torch.Generator().manual_seed(50 + i)
        recs.append({"frames": torch.randint(0, 256, (n, h * 3 // 2, w), generator=g, dtype=torch.uint8).to(DEV),
                     "wav": (0.1 * torch.randn(n * PER, generator=g)).to(DEV)})
    return {"cfg": cfg, "predictor": predictor, "recs": recs, "yuv": recs[0]["frames"], "wav": recs[0]["wav"]}


@pytest.mark.parametrize("layout", Q.FORMATS)
def test_predict_video_and_render_track(env, layout):
    p, yuv, wav, fmt = env["predictor"], env["yuv"], env["wav"], fmt_of(layout)
    kw = dict(stride=STRIDE, batch=BATCH, overlay=True, fill="linear")
    rgb_run = p.predict_video(yuv, wav, **kw, **fmt)
    run = p.predict_video(yuv, wav, overlay_format=layout, **kw, **fmt)
    same_but_overlay(run, rgb_run)
    assert rgb_run["overlay"].shape == (N, H, W, 3) and run["overlay"].shape == yuv.shape and run["overlay"].dtype == torch.uint8
    want, M = composed(yuv, rgb_run["overlay"], p.render_track(black_like(N, H, W), rgb_run, alpha=1.0), layout)
    drawn = M.any(axis=(1, 2))
    assert 0 < drawn.sum() < N and (M.sum(axis=(1, 2))[drawn] < H * W).all()          # 64 x 80: the crop leaves the sides out
    assert np.array_equal(run["overlay"].cpu().numpy(), want)
    assert torch.equal(run["overlay"][~torch.from_numpy(drawn).to(DEV)], yuv[~torch.from_numpy(drawn).to(DEV)])
    # "rgb24" and None are today's path
    assert torch.equal(p.predict_video(yuv, wav, overlay_format="rgb24", **kw, **fmt)["overlay"], rgb_run["overlay"])
    # render_track: the whole, in chunks, into a given output, in place
    for chunk in (None, 7):
        assert np.array_equal(p.render_track(yuv, run, chunk=chunk, out_format=layout, **fmt).cpu().numpy(), want), chunk
    out = torch.full_like(yuv, 3)
    assert p.render_track(yuv, run, out=out, chunk=33, out_format=layout, **fmt) is out and np.array_equal(out.cpu().numpy(), want)
    work = yuv.clone()
    assert p.render_track(work, run, out=work, chunk=40, out_format=layout, **fmt) is work
    assert np.array_equal(work.cpu().numpy(), want)
    # other alpha and radius
    D = p.render_track(yuv, run, alpha=0.7, radius=9, **fmt)
    want2, _ = composed(yuv, D, p.render_track(black_like(N, H, W), run, alpha=1.0, radius=9), layout)
    assert np.array_equal(p.render_track(yuv, run, alpha=0.7, radius=9, out_format=layout, **fmt).cpu().numpy(), want2)


def test_render_attention_and_render_attention_track(env):
    p, yuv, wav, layout = env["predictor"], env["yuv"], env["wav"], "nv12"
    fmt = fmt_of(layout)
    T = int(env["cfg"].DATA.NUM_FRAMES)
    pick = torch.arange(0, 2 * T * 5, 5, device=DEV).view(2, T)
    clips = yuv[pick].contiguous()                                                     # (2, T, 96, 80)
    w = wav[:2 * 40000].view(2, 40000)
    fidx = (torch.arange(T, device=DEV, dtype=torch.float32) * 5)[None].expand(2, T).contiguous()
    res = p.predict(clips, w, fidx, 60.0, attention=True, **fmt)
    for head in (1, None):
        D = p.render_attention(clips, res, head=head, points=res["points"], **fmt)
        black = p.render_attention(torch.zeros(2, T, H, W, 3, dtype=torch.uint8, device=DEV), res, head=head, alpha=1.0,
                                   points=res["points"])
        want, M = composed(clips.view(2 * T, H * 3 // 2, W), D.view(2 * T, H, W, 3), black.view(2 * T, H, W, 3), layout)
        assert M.any()
        got = p.render_attention(clips, res, head=head, points=res["points"], out_format=layout, **fmt)
        assert got.shape == clips.shape and np.array_equal(got.view(2 * T, H * 3 // 2, W).cpu().numpy(), want), head
    work = clips.clone()                                                               # in place, the head mean (the last `want`)
    assert p.render_attention(work, res, points=res["points"], out=work, out_format=layout, **fmt) is work
    assert np.array_equal(work.view(2 * T, H * 3 // 2, W).cpu().numpy(), want)
    # the attention track of a recording
    track = p.predict_video(yuv, wav, stride=STRIDE, batch=BATCH, attention_track=True, fill="hold", **fmt)
    for head, chunk in ((None, None), (0, 7)):
        D = p.render_attention_track(yuv, track, head=head, points=track["points"], **fmt)
        black = p.render_attention_track(black_like(N, H, W), track, head=head, points=track["points"], alpha=1.0)
        want, M = composed(yuv, D, black, layout)
        drawn = M.any(axis=(1, 2))
        assert 0 < drawn.sum() < N
        got = p.render_attention_track(yuv, track, head=head, points=track["points"], chunk=chunk, out_format=layout, **fmt)
        assert got.shape == yuv.shape and np.array_equal(got.cpu().numpy(), want), (head, chunk)
    work = yuv.clone()
    assert p.render_attention_track(work, track, head=0, points=track["points"], out=work, out_format=layout, **fmt) is work
    assert np.array_equal(work.cpu().numpy(), want)


def _replay_stream(stream, frames, wav, k=13):
    rows = []
    for a in range(0, frames.shape[0], k):
        b = min(a + k, frames.shape[0])
        rows.append(stream.push_live(frames[a:b], wav[a * PER:b * PER])[1])
    return {key: torch.cat([r[key] for r in rows], dim=0) for key in rows[0]}


@pytest.mark.parametrize("layout", Q.FORMATS)
def test_live_stream(env, layout):
    p, yuv, wav, fmt = env["predictor"], env["yuv"], env["wav"], fmt_of(layout)
    kw = dict(stride=STRIDE, live="linear", overlay=True, alpha=0.5, radius=3)
    a = _replay_stream(p.stream(overlay_format=layout, **kw, **fmt), yuv, wav)
    b = _replay_stream(p.stream(**kw, **fmt), yuv, wav)
    same_but_overlay(a, b)
    assert tuple(b["overlay"].shape) == (N, H, W, 3) and tuple(a["overlay"].shape) == tuple(yuv.shape)
    want, M = composed(yuv, b["overlay"], p.render_track(black_like(N, H, W), b, alpha=1.0, radius=3), layout)
    assert np.array_equal(a["overlay"].cpu().numpy(), want)
    nothing = a["neighbours"][:, 0] < 0
    assert 0 < int(nothing.sum()) < N and torch.equal(a["overlay"][nothing], yuv[nothing])
    assert not torch.equal(a["overlay"][~nothing], yuv[~nothing])
    s = p.stream(overlay_format=layout, **kw, **fmt)
    s.push_live(yuv[:2], None)
    empty = s.push_live(None, wav[:0])[1]
    assert tuple(empty["overlay"].shape) == (0, H * 3 // 2, W)


def test_live_group_of_two_slots(env):
    p, recs, layout = env["predictor"], env["recs"], "nv12"
    fmt = fmt_of(layout)
    kw = dict(stride=STRIDE, overlay=True, alpha=0.5, radius=3)

    def replay(group):
        lives = {0: [], 1: []}
        for a in range(0, N, 13):
            b = min(a + 13, N)
            rows = group.push_live({i: (recs[i]["frames"][a:b], recs[i]["wav"][a * PER:b * PER]) for i in range(2)})[1]
            for i in range(2):
                lives[i].append(rows[i])
        return {i: {k: torch.cat([r[k] for r in rs], dim=0) for k in rs[0]} for i, rs in lives.items()}

    got = replay(p.live_group(2, "linear", overlay_format=layout, **kw, **fmt))
    ref = replay(p.live_group(2, "linear", **kw, **fmt))
    for i, (n, h, w) in enumerate(SHAPES):
        same_but_overlay(got[i], ref[i])
        frames = recs[i]["frames"]
        assert tuple(ref[i]["overlay"].shape) == (n, h, w, 3) and tuple(got[i]["overlay"].shape) == tuple(frames.shape)
        want, M = composed(frames, ref[i]["overlay"], p.render_track(black_like(n, h, w), ref[i], alpha=1.0, radius=3), layout)
        assert M.any() and np.array_equal(got[i]["overlay"].cpu().numpy(), want), i
    group = p.live_group(2, "hold", overlay_format=layout, **kw, **fmt)
    group.push_live({0: (recs[0]["frames"][:2], None), 1: (recs[1]["frames"][:2], None)})
    empty = group.push_live({0: (None, None), 1: (None, recs[1]["wav"][:0])})[1]
    assert tuple(empty[0]["overlay"].shape) == (0, 96, 80) and tuple(empty[1]["overlay"].shape) == (0, 72, 64)


def test_refusals(env):
    p, yuv, wav = env["predictor"], env["yuv"], env["wav"]
    fmt = fmt_of("nv12")
    track = p.predict_video(yuv, wav, stride=STRIDE, batch=BATCH, **fmt)
    rgb = inputs.yuv_to_rgb(yuv, **fmt)
    with pytest.raises(ValueError, match="packed RGB"):                                 # a 4:2:0 out_format on RGB frames
        p.render_track(rgb, track, out_format="nv12")
    with pytest.raises(ValueError, match="layout of the frames"):                      # a layout mismatch
        p.render_track(yuv, track, out_format="i420", **fmt)
    with pytest.raises(ValueError, match="out_format must be"):
        p.render_track(yuv, track, out_format="yuv444", **fmt)
    with pytest.raises(ValueError, match="packed RGB"):
        p.predict_video(rgb, wav, stride=STRIDE, batch=BATCH, overlay=True, overlay_format="nv12")
    with pytest.raises(ValueError, match="layout of the frames"):
        p.predict_video(yuv, wav, stride=STRIDE, batch=BATCH, overlay=True, overlay_format="i420", **fmt)
    with pytest.raises(ValueError, match="overlay=True"):
        p.predict_video(yuv, wav, stride=STRIDE, batch=BATCH, overlay_format="nv12", **fmt)
    with pytest.raises(ValueError, match="packed RGB"):
        p.stream(stride=STRIDE, live="hold", overlay=True, overlay_format="nv12")
    with pytest.raises(ValueError, match="layout of the frames"):
        p.stream(stride=STRIDE, live="hold", overlay=True, overlay_format="nv12", pixel_format="i420")
    with pytest.raises(ValueError, match="overlay=True"):
        p.stream(stride=STRIDE, live="hold", overlay_format="nv12", **fmt)
    with pytest.raises(ValueError, match="packed RGB"):
        p.live_group(2, "hold", overlay=True, overlay_format="i420")
    with pytest.raises(ValueError, match="layout of the frames"):
        p.live_group(2, "hold", overlay=True, overlay_format="i420", **fmt)
    with pytest.raises(ValueError, match="in place"):                                   # out overlapping the frames without being them
        p.render_track(yuv[:-1], {k: track[k][:-1] for k in ("rescaled", "points")}, out=yuv[1:], out_format="nv12", **fmt)
    with pytest.raises(ValueError, match="out must"):
        p.render_track(yuv, track, out=torch.empty(N, H, W, 3, dtype=torch.uint8, device=DEV), out_format="nv12", **fmt)
    res = {"attention_maps": torch.zeros(1, 3, 8, 8, 8, device=DEV)}
    with pytest.raises(ValueError, match="packed RGB"):
        p.render_attention(torch.zeros(1, 8, H, W, 3, dtype=torch.uint8, device=DEV), res, out_format="nv12")
    with pytest.raises(ValueError, match="layout of the frames"):
        p.render_attention_track(yuv, {"attention_maps": torch.zeros(N, 3, 8, 8, device=DEV),
                                       "attention_count": torch.zeros(N, dtype=torch.int32, device=DEV)}, out_format="i420", **fmt)
