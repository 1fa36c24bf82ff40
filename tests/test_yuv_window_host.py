"""Decoder surfaces on the host: inputs.check_window refuses what the definition rules out and names the value;
inputs.yuv_window (the repack, the oracle of every window= keyword) equals a numpy restatement for both layouts;
yuv_to_rgb_host(window=) equals yuv_to_rgb_host of the repack on every shared case, both matrices and ranges; the header declares
the six *_win entry points, lib.py binds them, both libraries export them and the ABI number stays 14."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from csts_amd import inputs, lib  # noqa: E402

LAYOUTS = ("nv12", "i420")
# (Hs, Ws, N, window): the shared cases of the surface tests
CASES = [(40, 96, 3, (0, 0, 36, 70)),        # the decoder case: pitch and coded height only
         (40, 96, 3, (2, 6, 30, 50)),        # left no multiple of 16, left / 2 odd, W no multiple of 16
         (40, 96, 3, (4, 26, 36, 70)),       # touches the right and bottom edges: the last byte read is the tensor's last
         (40, 96, 3, (0, 0, 40, 96)),        # the whole surface
         (8, 4160, 1, (2, 34, 4, 4100))]     # a row wider than an overlay tile and a staging pass
WIN_SYMBOLS = ("csts_yuv_to_rgb_win", "csts_yuv_to_rgb_win_host", "csts_spatial_sample_yuv_win", "csts_clip_sample_yuv_win",
               "csts_stream_ingest_yuv_win", "csts_gaze_overlay_yuv_win")


def surface(Hs, Ws, N, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (N, Hs * 3 // 2, Ws), dtype=np.uint8)


def repack_numpy(x, layout, window):
    """The window of surfaces x (N, Hs * 3 / 2, Ws) as tight pictures, byte by byte from the definition."""
    top, left, H, W = window
    N, rows, Ws = x.shape
    Hs = rows // 3 * 2
    flat = x.reshape(N, -1)
    out = np.empty((N, H * 3 // 2 * W), dtype=np.uint8)
    for y in range(H):
        out[:, y * W:(y + 1) * W] = flat[:, (top + y) * Ws + left:(top + y) * Ws + left + W]
    c0, o0 = Hs * Ws, H * W
    for cy in range(H // 2):
        r = top // 2 + cy
        if layout == "nv12":
            out[:, o0 + cy * W:o0 + (cy + 1) * W] = flat[:, c0 + r * Ws + left:c0 + r * Ws + left + W]
        else:
            hs, hw = Ws // 2, W // 2
            for plane in range(2):
                src = c0 + plane * (Hs // 2) * hs + r * hs + left // 2
                dst = o0 + plane * (H // 2) * hw + cy * hw
                out[:, dst:dst + hw] = flat[:, src:src + hw]
    return out.reshape(N, H * 3 // 2, W)


@pytest.mark.parametrize("window,word", [((1, 0, 2, 2), "top 1"), ((0, 3, 2, 2), "left 3"), ((0, 0, 5, 2), "H 5"),
                                         ((0, 0, 2, 7), "W 7"), ((-2, 0, 2, 2), "top -2"), ((0, -4, 2, 2), "left -4"),
                                         ((0, 0, -2, 2), "H -2"), ((0, 0, 2, -6), "W -6"), ((6, 0, 36, 2), "42"),
                                         ((0, 28, 2, 70), "98"), ((0, 0, 0, 2), "H 0")])
def test_check_window_names_the_offending_value(window, word):
    with pytest.raises(ValueError, match=re.escape(word)):
        inputs.check_window((3, 60, 96), "nv12", window)


def test_check_window_rules():
    assert inputs.check_window((3, 60, 96), "i420", None) is None
    assert inputs.check_window((3, 60, 96), "i420", [2, 6, 30, 50]) == (2, 6, 30, 50)
    assert inputs.check_window((3, 60, 96), "nv12", np.array([4, 26, 36, 70])) == (4, 26, 36, 70)
    with pytest.raises(ValueError, match="rgb24"):
        inputs.check_window((3, 40, 96, 3), "rgb24", (0, 0, 2, 2))
    assert inputs.check_window((3, 40, 96, 3), "rgb24", None) is None
    for bad in ((0, 0, 2), (0, 0, 2.5, 2), "abcd", 7):
        with pytest.raises(ValueError, match="four integers"):
            inputs.check_window((3, 60, 96), "nv12", bad)
    with pytest.raises(ValueError, match=str(inputs.YUV_MAX_WS)):
        inputs.check_window((1, 3, inputs.YUV_MAX_WS + 2), "nv12", (0, 0, 2, 2))
    with pytest.raises(ValueError, match="tight"):
        inputs.rgb_to_yuv(torch.zeros(1, 2, 2, 3, dtype=torch.uint8), "nv12", window=(0, 0, 2, 2))
    for refuse in (inputs.group_ingest, inputs.batch_sample):
        with pytest.raises(ValueError, match="no window"):
            refuse(*([None] * (3 if refuse is inputs.group_ingest else 6)), window=(0, 0, 2, 2))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", CASES)
def test_yuv_window_is_the_numpy_restatement(layout, case):
    Hs, Ws, N, window = case
    x = surface(Hs, Ws, N)
    want = repack_numpy(x, layout, window)
    got = inputs.yuv_window(x, layout, window)
    assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want)
    t = inputs.yuv_window(torch.from_numpy(x), layout, window)
    assert t.is_contiguous() and np.array_equal(t.numpy(), want)
    lead = inputs.yuv_window(torch.from_numpy(x)[None], layout, window)              # leading dimensions stay
    assert tuple(lead.shape) == (1,) + want.shape and np.array_equal(lead[0].numpy(), want)
    assert inputs.yuv_window(x, layout, None) is x
    if window == (0, 0, Hs, Ws):
        assert np.array_equal(got, x)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", CASES)
def test_yuv_to_rgb_host_window_equals_the_repack(layout, case):
    Hs, Ws, N, window = case
    x = surface(Hs, Ws, N, seed=1)
    tight = inputs.yuv_window(x, layout, window)
    for matrix in ("bt601", "bt709"):
        for full_range in (False, True):
            got = inputs.yuv_to_rgb_host(x, layout, matrix, full_range, window=window)
            want = inputs.yuv_to_rgb_host(tight, layout, matrix, full_range)
            assert got.shape == (N, window[2], window[3], 3) and np.array_equal(got, want), (matrix, full_range)
    # padding is never read: other bytes around the same window give the same picture
    other = surface(Hs, Ws, N, seed=2)
    top, left, H, W = window
    flat = np.zeros((Hs * 3 // 2 * Ws,), dtype=bool)
    probe = np.arange(Hs * 3 // 2 * Ws, dtype=np.int64).reshape(1, Hs * 3 // 2, Ws)      # which bytes does the repack take?
    flat[inputs.yuv_window(probe, layout, window).reshape(-1)] = True
    mask = flat.reshape(Hs * 3 // 2, Ws)
    mixed = np.where(mask, x, other)
    assert np.array_equal(inputs.yuv_to_rgb_host(mixed, layout, window=window), inputs.yuv_to_rgb_host(x, layout, window=window))
    assert np.array_equal(inputs.yuv_to_rgb_host(x, layout, window=None), inputs.yuv_to_rgb_host(x, layout))


def test_the_c_entry_refuses_a_bad_window_and_writes_nothing():
    h = lib.load()
    x = surface(8, 16, 1)
    for H, W, Hs, Ws, top, left in ((4, 4, 8, 16, 1, 0), (4, 4, 8, 16, 0, 3), (4, 4, 8, 16, 6, 0), (4, 4, 8, 16, 0, 14),
                                    (0, 4, 8, 16, 0, 0), (4, 4, 8, 16, -2, 0), (2, 2, 2, lib_max_ws() + 2, 0, 0)):
        out = np.full((1, max(H, 1), W, 3), 7, dtype=np.uint8)
        assert h.csts_yuv_to_rgb_win_host(x.ctypes.data, out.ctypes.data, 1, H, W, Hs, Ws, top, left, lib.YUV_NV12, 0, 0) == -1
        assert (out == 7).all()


def lib_max_ws():
    hdr = open(os.path.join(ROOT, "include", "csts_hip.h")).read()
    limit = int(re.search(r"#define CSTS_YUV_MAX_WS (\d+)", hdr).group(1))
    assert limit == inputs.YUV_MAX_WS
    return limit


def test_abi_and_symbols():
    hdr = open(os.path.join(ROOT, "include", "csts_hip.h")).read()
    assert int(re.search(r"#define CSTS_ABI_VERSION (\d+)", hdr).group(1)) == lib.ABI_VERSION == 14
    for name in WIN_SYMBOLS:
        assert re.search(r"\bint " + name + r"\(", hdr), name
        assert name in lib.SYMBOLS, name
        args = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr).group(1)
        assert re.search(r"int H, int W,\s+int Hs, int Ws,\s+int top,\s+int left", args), name     # next to H, W
        assert len(lib.SYMBOLS[name][1]) == len(args.split(",")), name
    for path in lib._PATHS.values():
        handle = ctypes.CDLL(path)
        for name in WIN_SYMBOLS:
            assert hasattr(handle, name), (path, name)
