"""Decoder surfaces on the device: every function that takes window= equals, bit for bit (torch.equal), the same function on
inputs.yuv_window of the surface -- yuv_to_rgb, spatial_sample, clip_sample, stream_ingest and the 4:2:0 overlay -- on surfaces of
40 x 96 (N = 3) and 8 x 4160 (N = 1), both layouts; no byte outside the window takes part in a result, the overlay leaves every
byte outside the window as it was, the whole surface is today's call, and a bad window is refused before anything is written."""
import ctypes as C
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from csts_amd import inputs, ops, lib as L  # noqa: E402

DEV = torch.device("cuda:0")
LAYOUTS = ("nv12", "i420")
SMALL = [(40, 96, 3, (0, 0, 36, 70)),        # the decoder case: pitch and coded height only
         (40, 96, 3, (2, 6, 30, 50)),        # left no multiple of 16, left / 2 odd, W no multiple of 16
         (40, 96, 3, (4, 26, 36, 70)),       # touches the right and bottom edges: the last byte read is the tensor's last
         (40, 96, 3, (0, 0, 40, 96))]        # the whole surface
WIDE = (8, 4160, 1, (2, 34, 4, 4100))        # wider than an overlay tile (crossed twice) and than a staging pass
VEC = (40, 96, 3, (4, 8, 32, 64))            # W, Ws, left multiples of 4: the overlay's 4-pixel path on a true window
FORMATS = [(m, r) for m in ("bt601", "bt709") for r in (False, True)]
_CACHE = {}


def surface(Hs, Ws, N, seed=0):
    key = (Hs, Ws, N, seed)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(100 + seed)
        _CACHE[key] = torch.randint(0, 256, (N, Hs * 3 // 2, Ws), generator=g, dtype=torch.uint8).to(DEV)
    return _CACHE[key]


def window_mask(Hs, Ws, layout, window):
    """bool (Hs * 3 / 2, Ws): the bytes of a surface the window is made of."""
    probe = torch.arange(Hs * 3 // 2 * Ws, dtype=torch.int64).view(1, Hs * 3 // 2, Ws)
    mask = torch.zeros(Hs * 3 // 2 * Ws, dtype=torch.bool)
    mask[inputs.yuv_window(probe, layout, window).reshape(-1)] = True
    return mask.view(Hs * 3 // 2, Ws).to(DEV)


def other_padding(x, Hs, Ws, layout, window):
    """A surface that agrees with x inside the window and holds other random bytes everywhere else."""
    return torch.where(window_mask(Hs, Ws, layout, window), x, surface(Hs, Ws, x.shape[0], seed=9))


def sample_params(B, H, W, S, flip):
    """Rows (new h, new w, y0, x0, flip): a downscale and an upscale, crops off centre."""
    rows = []
    for b in range(B):
        nh, nw = (max(S, H * 4 // 5), max(S, W * 4 // 5)) if b % 2 == 0 else (H + 7, W + 5)
        rows.append([nh, nw, (nh - S) // 3, (nw - S) * 2 // 3, flip])
    return torch.tensor(rows, dtype=torch.int32, device=DEV)


# ---- the equation ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", SMALL + [WIDE])
def test_yuv_to_rgb(layout, case):
    Hs, Ws, N, window = case
    x = surface(Hs, Ws, N)
    tight = inputs.yuv_window(x, layout, window)
    y = other_padding(x, Hs, Ws, layout, window)
    for matrix, full_range in FORMATS:
        want = inputs.yuv_to_rgb(tight, layout, matrix, full_range)
        got = inputs.yuv_to_rgb(x, layout, matrix, full_range, window=window)
        assert got.shape == (N, window[2], window[3], 3) and torch.equal(got, want), (matrix, full_range)
        assert torch.equal(inputs.yuv_to_rgb(y, layout, matrix, full_range, window=window), want)      # padding is never read
    out = torch.full((N * window[2] * window[3] * 3 + 5,), 9, dtype=torch.uint8, device=DEV)            # out at an odd byte
    view = out[3:-2].view(N, window[2], window[3], 3)
    assert inputs.yuv_to_rgb(x, layout, window=window, out=view) is view
    assert torch.equal(view, inputs.yuv_to_rgb(tight, layout)) and (out[:3] == 9).all() and (out[-2:] == 9).all()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", SMALL)
@pytest.mark.parametrize("S", [16, 18])
def test_spatial_sample(layout, case, S):
    Hs, Ws, N, window = case
    x = surface(Hs, Ws, N).view(1, N, Hs * 3 // 2, Ws)
    tight = inputs.yuv_window(x, layout, window)
    y = other_padding(x[0], Hs, Ws, layout, window)[None]
    fmt = dict(pixel_format=layout, matrix="bt709" if layout == "nv12" else "bt601", full_range=layout == "i420")
    for flip in (0, 1):
        par = sample_params(1, window[2], window[3], S, flip)
        want = inputs.spatial_sample(tight, par, S, **fmt)
        assert torch.isfinite(want).all()
        assert torch.equal(inputs.spatial_sample(x, par, S, window=window, **fmt), want), flip
        assert torch.equal(inputs.spatial_sample(y, par, S, window=window, **fmt), want), flip
    # the three frames as three clips, and the rule that derives the parameters from the window's size
    xb, tb = x.view(N, 1, Hs * 3 // 2, Ws), tight.view(N, 1, window[2] * 3 // 2, window[3])
    par = sample_params(N, window[2], window[3], S, 0)
    assert torch.equal(inputs.spatial_sample(xb, par, S, window=window, **fmt), inputs.spatial_sample(tb, par, S, **fmt))
    lab = torch.rand(N, 1, 2, dtype=torch.float64, device=DEV)
    got = inputs.spatial_sampling(xb, lab, S, train=False, spatial_idx=1, return_params=True, window=window, **fmt)
    want = inputs.spatial_sampling(tb, lab, S, train=False, spatial_idx=1, return_params=True, **fmt)
    assert all(torch.equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", SMALL)
def test_clip_sample(layout, case):
    Hs, Ws, N, window = case
    x = surface(Hs, Ws, N)
    tight = inputs.yuv_window(x, layout, window)
    y = other_padding(x, Hs, Ws, layout, window)
    idx = torch.tensor([[-2, 0, 1, N - 1], [N - 1, N, N + 5, -1]], dtype=torch.int32, device=DEV)     # clamped to [0, N - 1]
    fmt = dict(pixel_format=layout, matrix="bt601" if layout == "nv12" else "bt709", full_range=layout == "nv12")
    for S in (16, 18):
        par = sample_params(2, window[2], window[3], S, 0)
        par[1, 4] = 1
        want = inputs.clip_sample(tight, idx, par, S, **fmt)
        assert torch.isfinite(want).all()
        assert torch.equal(inputs.clip_sample(x, idx, par, S, window=window, **fmt), want), S
        assert torch.equal(inputs.clip_sample(y, idx, par, S, window=window, **fmt), want), S


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", SMALL)
def test_stream_ingest(layout, case):
    Hs, Ws, N, window = case
    x = surface(Hs, Ws, N)
    tight = inputs.yuv_window(x, layout, window)
    y = other_padding(x, Hs, Ws, layout, window)
    S, R = 18, 5
    par = sample_params(1, window[2], window[3], S, 0)[0]
    pairs = torch.tensor([[N - 1, 3], [0, 1]], dtype=torch.int32, device=DEV)
    fmt = dict(pixel_format=layout, matrix="bt709", full_range=False)
    rings = []
    for src, kw in ((tight, {}), (x, {"window": window}), (y, {"window": window})):
        ring = torch.full((R, 3, S, S), -7.0, dtype=torch.float32, device=DEV)
        assert inputs.stream_ingest(src, pairs, par, ring, **fmt, **kw) is ring
        rings.append(ring)
    assert torch.equal(rings[1], rings[0]) and torch.equal(rings[2], rings[0])
    assert torch.isfinite(rings[0][[1, 3]]).all() and (rings[0][[0, 2, 4]] == -7.0).all()          # unnamed slots untouched
    want = inputs.clip_sample(tight, torch.tensor([[N - 1]], dtype=torch.int32, device=DEV), par[None], S, **fmt)
    assert torch.equal(rings[1][3], want[0, :, 0])


# ---- the overlay -----------------------------------------------------------------------------------------------------------------

def overlay_args(N, H, W, wide):
    """maps, the host params row, centres (X, Y) in window pixels and the crop size.  The small cases draw a crop inside the
    picture, a marker inside and one at its edge, and leave the last frame alone (negative centre); the wide case draws it all."""
    g = torch.Generator().manual_seed(5)
    maps = torch.rand(N, 4, 4, generator=g).to(DEV)
    if wide:
        return maps, [4, 4, 0, 0, 0], torch.tensor([[W // 2, 1]], dtype=torch.int32, device=DEV), 4
    S = 16
    nh, nw = max(S, H * 3 // 4), max(S, W * 3 // 4)
    centers = torch.tensor([[W // 2, H // 2], [W - 1, 1], [-1, -1]], dtype=torch.int32, device=DEV)[:N]
    return maps, [nh, nw, (nh - S) // 2, (nw - S) // 3, 0], centers, S


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", SMALL + [WIDE, VEC])
def test_overlay(layout, case):
    Hs, Ws, N, window = case
    top, left, H, W = window
    x = surface(Hs, Ws, N)
    tight = inputs.yuv_window(x, layout, window)
    mask = window_mask(Hs, Ws, layout, window)
    maps, row, centers, S = overlay_args(N, H, W, case is WIDE)
    for matrix, full_range in (("bt601", False), ("bt709", True)):
        fmt = dict(pixel_format=layout, matrix=matrix, full_range=full_range)
        kw = dict(centers=centers, alpha=0.4, radius=3)
        want = ops.gaze_overlay_yuv(tight, maps, row, S, **fmt, **kw)
        assert not torch.equal(want, tight)                                          # something is drawn
        got = ops.gaze_overlay_yuv(x, maps, row, S, window=window, **fmt, **kw)
        assert got.shape == x.shape and got.data_ptr() != x.data_ptr()
        assert torch.equal(inputs.yuv_window(got, layout, window), want)
        assert torch.equal(torch.where(mask, x, got), x)                             # every byte outside the window is the input's
        # in place: the same bytes, written where they were
        buf = x.clone()
        assert ops.gaze_overlay_yuv(buf, maps, row, S, window=window, out=buf, **fmt, **kw) is buf and torch.equal(buf, got)
        # into a given tensor that held something else
        out = torch.full_like(x, 77)
        assert ops.gaze_overlay_yuv(x, maps, row, S, window=window, out=out, **fmt, **kw) is out and torch.equal(out, got)
        # padding is never read
        y = other_padding(x, Hs, Ws, layout, window)
        assert torch.equal(inputs.yuv_window(ops.gaze_overlay_yuv(y, maps, row, S, window=window, **fmt, **kw), layout, window), want)
        if N == 3:                                                                   # negative centre: the frame comes back whole
            assert torch.equal(got[2], x[2])
    # no frame drawn at all: negative centres everywhere -> the whole surface byte for byte, in place and not
    none = torch.full((N, 2), -1, dtype=torch.int32, device=DEV)
    assert torch.equal(ops.gaze_overlay_yuv(x, maps, row, S, layout, centers=none, window=window), x)
    buf = x.clone()
    ops.gaze_overlay_yuv(buf, maps, row, S, layout, centers=none, window=window, out=buf)
    assert torch.equal(buf, x)


# ---- the whole surface is today's call -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", LAYOUTS)
def test_whole_surface(layout):
    Hs, Ws, N = 40, 96, 3
    x = surface(Hs, Ws, N)
    whole = (0, 0, Hs, Ws)
    fmt = dict(pixel_format=layout, matrix="bt601", full_range=False)
    idx = torch.tensor([[0, 2, 1]], dtype=torch.int32, device=DEV)
    par = sample_params(1, Hs, Ws, 18, 1)
    pairs = torch.tensor([[1, 0]], dtype=torch.int32, device=DEV)
    maps, row, centers, S = overlay_args(N, Hs, Ws, False)

    def ring(**kw):
        return inputs.stream_ingest(x, pairs, par[0], torch.zeros(2, 3, 18, 18, device=DEV), **fmt, **kw)

    for kw in ({"window": None}, {"window": whole}):
        assert torch.equal(inputs.yuv_to_rgb(x, layout, **kw), inputs.yuv_to_rgb(x, layout))
        assert torch.equal(inputs.spatial_sample(x[None], par, 18, **fmt, **kw), inputs.spatial_sample(x[None], par, 18, **fmt))
        assert torch.equal(inputs.clip_sample(x, idx, par, 18, **fmt, **kw), inputs.clip_sample(x, idx, par, 18, **fmt))
        assert torch.equal(ring(**kw), ring())
        want = ops.gaze_overlay_yuv(x, maps, row, S, centers=centers, **fmt)
        assert torch.equal(ops.gaze_overlay_yuv(x, maps, row, S, centers=centers, **fmt, **kw), want)
        buf = x.clone()
        ptr = buf.data_ptr()
        assert ops.gaze_overlay_yuv(buf, maps, row, S, centers=centers, out=buf, **fmt, **kw) is buf
        assert buf.data_ptr() == ptr and torch.equal(buf, want)


# ---- refusals: before any launch, nothing written --------------------------------------------------------------------------------

BAD = [(1, 0, 30, 50), (0, 3, 30, 50), (0, 0, 31, 50), (0, 0, 30, 51), (-2, 0, 30, 50), (12, 0, 30, 50), (0, 48, 30, 50),
       (0, 0, 0, 50)]


@pytest.mark.parametrize("window", BAD)
def test_python_refusals(window):
    Hs, Ws, N = 40, 96, 3
    x = surface(Hs, Ws, N)
    H, W = max(window[2], 2), max(window[3], 2)
    par = torch.tensor([[16, 16, 0, 0, 0]], dtype=torch.int32, device=DEV)
    idx = torch.zeros(1, 1, dtype=torch.int32, device=DEV)
    ring = torch.full((2, 3, 16, 16), -7.0, device=DEV)
    out = torch.full_like(x, 77)
    rgb = torch.full((N, H, W, 3), 77, dtype=torch.uint8, device=DEV)
    maps = torch.rand(N, 4, 4, device=DEV)
    torch.cuda.synchronize()
    calls = [lambda: inputs.yuv_to_rgb(x, "nv12", window=window, out=rgb),
             lambda: inputs.spatial_sample(x[None], par, 16, pixel_format="nv12", window=window),
             lambda: inputs.clip_sample(x, idx, par, 16, pixel_format="i420", window=window),
             lambda: inputs.stream_ingest(x, torch.zeros(1, 2, dtype=torch.int32, device=DEV), par[0], ring, pixel_format="nv12",
                                          window=window),
             lambda: ops.gaze_overlay_yuv(x, maps, [16, 16, 0, 0, 0], 16, "i420", window=window, out=out)]
    for call in calls:
        with pytest.raises(ValueError, match="window"):
            call()
    assert (out == 77).all() and (rgb == 77).all() and (ring == -7.0).all()


def test_rgb24_and_group_refusals():
    rgb = torch.zeros(1, 2, 8, 8, 3, dtype=torch.uint8, device=DEV)
    par = torch.tensor([[8, 8, 0, 0, 0]], dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="rgb24"):
        inputs.spatial_sample(rgb, par, 8, window=(0, 0, 4, 4))
    with pytest.raises(ValueError, match="rgb24"):
        inputs.clip_sample(rgb[0], torch.zeros(1, 2, dtype=torch.int32, device=DEV), par, 8, window=(0, 0, 4, 4))
    with pytest.raises(ValueError, match="rgb24"):
        inputs.stream_ingest(rgb[0], torch.zeros(1, 2, dtype=torch.int32, device=DEV), par[0],
                             torch.zeros(2, 3, 8, 8, device=DEV), window=(0, 0, 4, 4))
    with pytest.raises(ValueError, match="rgb24"):
        inputs.assemble_batch(rgb, None, None, 8.0, None, window=(0, 0, 4, 4))
    x = surface(40, 96, 3)
    with pytest.raises(ValueError, match="no window"):
        ops.group_gaze_overlay([(x, [16, 16, 0, 0, 0])], torch.zeros(3, 4, 4, device=DEV), None, 16, pixel_format="nv12",
                               window=(0, 0, 36, 70))
    with pytest.raises(ValueError, match="no window"):
        inputs.group_ingest([(x, [16, 16, 0, 0, 0])], [[0, 0, 0]], torch.zeros(2, 3, 16, 16, device=DEV), pixel_format="nv12",
                            window=(0, 0, 36, 70))


def test_c_entry_refusals_write_nothing():
    """The C ABI itself: -1 for a bad window, before any launch -- the outputs keep their bytes."""
    Hs, Ws, N, S = 40, 96, 3, 16
    x = surface(Hs, Ws, N)
    h = L.load()
    f3 = C.c_float * 3
    mean, std = f3(0.45, 0.45, 0.45), f3(0.225, 0.225, 0.225)
    par = torch.tensor([[16, 16, 0, 0, 0]], dtype=torch.int32, device=DEV)
    idx = torch.zeros(1, 1, dtype=torch.int32, device=DEV)
    pairs = torch.zeros(1, 2, dtype=torch.int32, device=DEV)
    maps = torch.rand(N, 4, 4, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    for top, left, H, W, ws in [(1, 0, 30, 50, Ws), (0, 3, 30, 50, Ws), (0, 0, 31, 50, Ws), (12, 0, 30, 50, Ws), (0, 48, 30, 50, Ws),
                                (0, 0, 0, 50, Ws), (-2, 0, 30, 50, Ws), (0, 0, 2, 2, 32770)]:
        rgb = torch.full((N, max(H, 2), W, 3), 77, dtype=torch.uint8, device=DEV)
        clip = torch.full((1, 3, 1, S, S), -7.0, device=DEV)
        ring = torch.full((2, 3, S, S), -7.0, device=DEV)
        out = torch.full_like(x, 77)
        p = [t.data_ptr() for t in (x, rgb, clip, ring, out, par, idx, pairs, maps)]
        assert h.csts_yuv_to_rgb_win(p[0], p[1], N, H, W, Hs, ws, top, left, L.YUV_NV12, 0, 0, stream) == -1
        assert h.csts_spatial_sample_yuv_win(p[0], p[5], p[2], 1, 1, H, W, Hs, ws, top, left, S, mean, std, L.YUV_NV12, 0, 0, stream) == -1
        assert h.csts_clip_sample_yuv_win(p[0], N, p[6], p[5], p[2], 1, 1, H, W, Hs, ws, top, left, S, mean, std, L.YUV_I420, 0, 0,
                                          stream) == -1
        assert h.csts_stream_ingest_yuv_win(p[0], N, H, W, Hs, ws, top, left, p[7], 1, p[5], p[3], 2, S, mean, std, L.YUV_NV12, 0, 0,
                                            stream) == -1
        assert h.csts_gaze_overlay_yuv_win(p[0], p[8], None, p[5], p[4], N, H, W, Hs, ws, top, left, S, 4, 4, 0.4, 3, L.YUV_I420, 0, 0,
                                           stream) == -1
        torch.cuda.synchronize()
        assert (rgb == 77).all() and (clip == -7.0).all() and (ring == -7.0).all() and (out == 77).all()
