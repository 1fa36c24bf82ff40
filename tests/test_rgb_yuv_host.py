"""rgb_to_yuv, the host side (no GPU): the four inverse coefficient tables against exact rationals, the C functions
(csts_rgb_to_yuv_host) against the numpy int64 restatement of the rule (tests/rgb_yuv_reference.py) on every byte triple, on seeded
random frames and on unaligned buffers of both layouts, the derived bound against the real-valued matrix, the exported symbols and
ABI version, and the argument errors.

Bounds.  C against the restatement: equality (the rule is integer).  Integer rule against floor(real matrix + 0.5): at most 1 -- a
coefficient is off by at most 2^-21, three terms of at most 255 (chroma: 1020 / 4) move the value before rounding by less than
4e-4, which changes the floor by at most one step.  Accumulator: the largest coefficient is 2^19 (the 0.5 of full-range chroma)
and the largest sum 1020, so with the rounding constant at most 524288 * 1020 + 2^21 = 2^29 (5.35e8 before the constant): int32
holds it."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import rgb_yuv_reference as Q  # noqa: E402
from csts_amd import inputs, lib  # noqa: E402

NEW_SYMBOLS = ("csts_rgb_to_yuv", "csts_rgb_to_yuv_host", "csts_gaze_overlay_yuv")
ISSUE_TABLES = {("bt601", False): [269262, 528618, 102662, -155423, -305128, 460551, 460551, -385654, -74897],
                ("bt601", True): [313524, 615514, 119538, -176932, -347356, 524288, 524288, -439026, -85262],
                ("bt709", False): [191455, 644067, 65019, -105533, -355018, 460551, 460551, -418321, -42230],
                ("bt709", True): [222927, 749942, 75707, -120138, -404150, 524288, 524288, -476214, -48074]}


@pytest.mark.parametrize("matrix,full_range", Q.TABLES)
def test_tables_are_the_rounded_rationals(matrix, full_range):
    want = Q.table(matrix, full_range)
    assert want == ISSUE_TABLES[(matrix, full_range)]
    assert list(inputs.RGB_TABLES[(matrix, full_range)]) == want
    hdr = open(os.path.join(ROOT, "include", "csts_hip.h")).read()
    stated = "{" + " | ".join(", ".join(str(v) for v in want[a:a + 3]) for a in (0, 3, 6)) + "}"
    assert stated in hdr                                                    # the header states the same numbers
    shared = open(os.path.join(ROOT, "csts_amd", "csrc", "yuv_shared.h")).read()
    assert "{" + ", ".join(str(v) for v in want) + ", " + ("0" if full_range else "16") + "}" in shared


@pytest.mark.parametrize("matrix,full_range", Q.TABLES)
def test_host_twin_is_exact_on_every_triple(matrix, full_range):
    """All 2^24 (R, G, B) triples as 2 x 2 blocks of four equal pixels through the C functions, both layouts: equal to the
    restatement, within 1 of the real-valued matrix rounded half up, accumulators inside int32."""
    worst_acc = worst_real = 0
    g, b = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
    for fmt in Q.FORMATS:
        seen = 0
        for r0 in range(0, 256, 16):
            rgb = Q.triple_frames(r0, r0 + 16)
            got = inputs.rgb_to_yuv_host(rgb, fmt, matrix, full_range)
            assert got.shape == (16, 768, 512) and got.dtype == np.uint8
            Y, U, V = Q.split(got, fmt)
            # one triple per block: (16, 256, 256, 3)
            tri = np.stack([np.broadcast_to(np.arange(r0, r0 + 16, dtype=np.int64)[:, None, None], (16, 256, 256)),
                            np.broadcast_to(g, (16, 256, 256)), np.broadcast_to(b, (16, 256, 256))], axis=-1)
            assert np.array_equal(rgb[:, 0::2, 0::2], tri) and np.array_equal(rgb[:, 1::2, 1::2], tri)
            wy, acc_y = Q.luma(tri, matrix, full_range)
            wu, wv, acc_c = Q.chroma(4 * tri, matrix, full_range)
            for dy in range(2):
                for dx in range(2):
                    assert np.array_equal(Y[:, dy::2, dx::2], wy), (fmt, r0)
            assert np.array_equal(U, wu) and np.array_equal(V, wv), (fmt, r0)
            ry, ru, rv = Q.real_yuv(tri, 4 * tri, matrix, full_range)
            worst_real = max(worst_real, int(np.abs(wy - ry).max()), int(np.abs(wu - ru).max()), int(np.abs(wv - rv).max()))
            worst_acc = max(worst_acc, acc_y, acc_c)
            seen += tri.shape[0] * 256 * 256
        assert seen == 1 << 24
    print(f"{matrix} full_range={full_range}: |accumulator| <= {worst_acc}, |integer - real| <= {worst_real}")
    assert worst_acc <= 1 << 29
    assert worst_real <= 1


@pytest.mark.parametrize("fmt", Q.FORMATS)
@pytest.mark.parametrize("matrix,full_range", Q.TABLES)
def test_host_twin_on_random_frames(fmt, matrix, full_range):
    """2 x 2, 6 x 10 and 4 x 1030 pixels, seeded: four different pixels a block, so the chroma sums are real sums."""
    rng = np.random.default_rng(11)
    for N, H, W in ((1, 2, 2), (3, 6, 10), (2, 4, 1030)):
        rgb = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
        got = inputs.rgb_to_yuv_host(rgb, fmt, matrix, full_range)
        assert got.shape == (N, H * 3 // 2, W) and np.array_equal(got, Q.to_yuv(rgb, fmt, matrix, full_range)), (H, W)
        one = inputs.rgb_to_yuv_host(rgb[0], fmt, matrix, full_range)      # any number of leading dimensions
        assert one.shape == (H * 3 // 2, W) and np.array_equal(one, got[0])
        lead = inputs.rgb_to_yuv_host(rgb[None], fmt, matrix, full_range)
        assert lead.shape == (1, N, H * 3 // 2, W) and np.array_equal(lead[0], got)


@pytest.mark.parametrize("fmt", Q.FORMATS)
def test_host_twin_on_odd_addresses(fmt):
    """Input and output both start 1 byte into their buffers (6 x 10 pixels: 180 bytes in, 90 out per frame)."""
    N, H, W = 3, 6, 10
    src = np.random.default_rng(5).integers(0, 256, N * H * W * 3 + 1, dtype=np.uint8)
    rgb = src[1:].reshape(N, H, W, 3)
    buf = np.full(N * H * W * 3 // 2 + 2, 0xA5, np.uint8)
    out = buf[1:-1].reshape(N, H * 3 // 2, W)
    assert rgb.ctypes.data % 2 == 1 and out.ctypes.data % 2 == 1
    rc = lib.load().csts_rgb_to_yuv_host(rgb.ctypes.data, out.ctypes.data, N, H, W, inputs.PIXEL_FORMATS.index(fmt), lib.YUV_BT601, 0)
    assert rc == 0
    assert np.array_equal(out, Q.to_yuv(rgb, fmt))
    assert buf[0] == 0xA5 and buf[-1] == 0xA5                               # nothing outside the output is written


def test_layouts_differ_only_in_where_chroma_lies():
    rgb = np.random.default_rng(3).integers(0, 256, (2, 6, 8, 3), dtype=np.uint8)
    a, b = inputs.rgb_to_yuv_host(rgb, "nv12"), inputs.rgb_to_yuv_host(rgb, "i420")
    for x, y in zip(Q.split(a, "nv12"), Q.split(b, "i420")):
        assert np.array_equal(x, y)
    # the round trip of a grey picture is the identity in limited range: R = G = B = v -> Y, 128, 128 -> v
    grey = np.repeat(np.arange(0, 256, dtype=np.uint8), 4 * 3).reshape(1, 2, 512, 3)
    back = inputs.yuv_to_rgb_host(inputs.rgb_to_yuv_host(grey, "nv12"), "nv12")
    assert int(np.abs(back.astype(np.int64) - grey).max()) <= 1


def test_abi_and_symbols():
    hdr = open(os.path.join(ROOT, "include", "csts_hip.h")).read()
    assert int(re.search(r"#define CSTS_ABI_VERSION (\d+)", hdr).group(1)) == lib.ABI_VERSION == 14
    for path in lib._PATHS.values():
        handle = ctypes.CDLL(path)
        for name in NEW_SYMBOLS:
            assert hasattr(handle, name), (path, name)
            assert name in lib.SYMBOLS and re.search(r"\b" + name + r"\(", hdr)


def test_c_entry_points_refuse_bad_arguments_on_the_host():
    h = lib.load()
    x, o = np.zeros(4 * 4 * 3, np.uint8), np.full(3 * 8, 7, np.uint8)
    ok = (x.ctypes.data, o.ctypes.data, 1, 4, 4)
    assert h.csts_rgb_to_yuv_host(*ok, lib.YUV_NV12, lib.YUV_BT601, 0) == 0
    o[:] = 7
    assert h.csts_rgb_to_yuv_host(*ok, 0, lib.YUV_BT601, 0) == -1                 # rgb24 is no 4:2:0 layout
    assert h.csts_rgb_to_yuv_host(*ok, 3, lib.YUV_BT601, 0) == -1                 # unknown layout
    assert h.csts_rgb_to_yuv_host(*ok, lib.YUV_I420, 2, 0) == -1                  # unknown matrix
    assert h.csts_rgb_to_yuv_host(x.ctypes.data, o.ctypes.data, 1, 3, 4, lib.YUV_NV12, 0, 0) == -1      # odd H
    assert b"even" in h.csts_last_error()
    assert h.csts_rgb_to_yuv_host(x.ctypes.data, o.ctypes.data, 1, 4, 3, lib.YUV_NV12, 0, 0) == -1      # odd W
    assert h.csts_rgb_to_yuv_host(None, o.ctypes.data, 1, 4, 4, lib.YUV_NV12, 0, 0) == -1
    assert h.csts_rgb_to_yuv_host(x.ctypes.data, None, 1, 4, 4, lib.YUV_NV12, 0, 0) == -1
    assert (o == 7).all()                                                           # a refused call writes nothing
    # the device entry points check their arguments before any launch
    assert h.csts_rgb_to_yuv(x.ctypes.data, o.ctypes.data, 1, 4, 5, lib.YUV_NV12, 0, 0, None) == -1     # odd W
    assert h.csts_rgb_to_yuv(x.ctypes.data, None, 1, 4, 4, lib.YUV_NV12, 0, 0, None) == -1
    assert h.csts_rgb_to_yuv(x.ctypes.data, x.ctypes.data, 1, 4, 4, lib.YUV_NV12, 0, 0, None) == -1     # overlap
    m, par = np.zeros(4, np.float32), np.zeros(5, np.int32)
    yuv = (o.ctypes.data, m.ctypes.data, None, par.ctypes.data)
    bad = [(yuv + (x.ctypes.data, 1, 3, 4, 4, 2, 2, 0.4, 5, lib.YUV_NV12, 0, 0, None), b"even"),            # odd H
           (yuv + (x.ctypes.data, 1, 4, 6, 4, 2, 2, 0.4, 5, 0, 0, 0, None), b"layout"),                     # rgb24
           (yuv + (x.ctypes.data, 1, 4, 8194, 4, 2, 2, 0.4, 5, lib.YUV_I420, 0, 0, None), b"8192"),         # too wide
           (yuv + (x.ctypes.data, 1, 4, 4, 4, 128, 128, 0.4, 5, lib.YUV_NV12, 0, 0, None), b"MAX_HW"),      # map too large
           (yuv + (o.ctypes.data + 8, 1, 4, 4, 4, 2, 2, 0.4, 5, lib.YUV_NV12, 0, 0, None), b"in place"),    # partial overlap
           (yuv + (None, 1, 4, 4, 4, 2, 2, 0.4, 5, lib.YUV_NV12, 0, 0, None), b"NULL")]
    for args, word in bad:
        assert h.csts_gaze_overlay_yuv(*args) == -1
        assert word in h.csts_last_error(), (word, h.csts_last_error())


def test_value_errors_come_before_the_device_check():
    import torch
    rgb = torch.zeros(2, 4, 6, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="pixel_format"):
        inputs.rgb_to_yuv(rgb, "yuv444")
    with pytest.raises(ValueError, match="matrix"):
        inputs.rgb_to_yuv(rgb, "nv12", matrix="bt2020")
    with pytest.raises(ValueError):
        inputs.rgb_to_yuv(rgb, "rgb24")
    with pytest.raises(ValueError, match="even"):
        inputs.rgb_to_yuv(torch.zeros(2, 5, 6, 3, dtype=torch.uint8), "nv12")
    with pytest.raises(ValueError, match="even"):
        inputs.rgb_to_yuv_host(np.zeros((4, 7, 3), np.uint8), "i420")
    with pytest.raises(ValueError, match="packed RGB"):
        inputs.rgb_to_yuv(torch.zeros(2, 6, 6, dtype=torch.uint8), "nv12")
    with pytest.raises(ValueError, match="out must"):
        inputs.rgb_to_yuv(rgb, "nv12", out=torch.zeros(2, 4, 6, dtype=torch.uint8))
    with pytest.raises(lib.CstsError, match="MI355X only"):
        inputs.rgb_to_yuv(rgb, "i420")
