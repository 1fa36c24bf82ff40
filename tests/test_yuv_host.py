"""4:2:0 YUV frames, the host side (no GPU): the four coefficient tables against exact rationals, the C pixel function
(csts_yuv_to_rgb_host) against the numpy int64 restatement of the rule (tests/yuv_reference.py) on every byte triple and on
unaligned recordings of both layouts, the derived bound against the real-valued matrix, the exported symbols and ABI version, and
the ValueErrors the Python layer raises on CPU tensors before it asks for a GPU.

Bounds.  C against the restatement: equality (the rule is integer).  Integer rule against clip(rint(real matrix)): at most 1, from
the coefficient rounding -- three terms of at most 255 * 2^-21 each move the value before rounding by less than 4e-4, which can
change rint() by at most one step.  Accumulator: below 5.74e8 (int32 holds it)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import yuv_reference as R  # noqa: E402
from csts_amd import datasets as D, inputs, lib  # noqa: E402

NEW_SYMBOLS = ("csts_yuv_to_rgb", "csts_yuv_to_rgb_host", "csts_spatial_sample_yuv", "csts_clip_sample_yuv", "csts_batch_sample_yuv")
ISSUE_TABLES = {("bt601", False): [1220945, 1673555, -410793, -852458, 2115221],
                ("bt601", True): [1048576, 1470104, -360853, -748826, 1858077],
                ("bt709", False): [1220945, 1879825, -223607, -558796, 2215014],
                ("bt709", True): [1048576, 1651297, -196424, -490864, 1945738]}


@pytest.mark.parametrize("matrix,full_range", R.TABLES)
def test_tables_are_the_rounded_rationals(matrix, full_range):
    want = R.table(matrix, full_range)
    assert want == ISSUE_TABLES[(matrix, full_range)]
    assert list(inputs.YUV_TABLES[(matrix, full_range)]) == want
    hdr = open(os.path.join(ROOT, "include", "csts_hip.h")).read()
    assert "{" + ", ".join(str(v) for v in want) + "}" in hdr             # the header states the same numbers


@pytest.mark.parametrize("matrix,full_range", R.TABLES)
def test_host_twin_is_exact_on_every_triple(matrix, full_range):
    """All 2^24 (Y, U, V) triples through the C pixel function, both layouts: equal to the restatement, within 1 of the real-valued
    matrix, accumulator inside int32."""
    worst_acc = worst_real = 0
    for fmt in R.FORMATS:
        frames = R.all_triples(fmt)
        got = inputs.yuv_to_rgb_host(frames, fmt, matrix, full_range)
        assert got.shape == (256, 128, 512, 3) and got.dtype == np.uint8
        seen = 0
        for a in range(0, 256, 32):                                         # in slabs: the int64 restatement is 24 bytes a pixel
            Y, U, V = R.planes(frames[a:a + 32], fmt)
            want, acc = R.pixels(Y, U, V, matrix, full_range)
            assert np.array_equal(got[a:a + 32], want), (fmt, a)
            worst_acc = max(worst_acc, acc)
            worst_real = max(worst_real, int(np.abs(want.astype(np.int64) - R.real_pixels(Y, U, V, matrix, full_range)).max()))
            if fmt == "nv12":
                code = (Y.astype(np.int64) << 16) | (U.astype(np.int64) << 8) | V
                seen += np.unique(code).size
        if fmt == "nv12":
            assert seen == 1 << 24                                          # the frames do hold every triple (slabs split by U)
    print(f"{matrix} full_range={full_range}: |accumulator| <= {worst_acc}, |integer - real| <= {worst_real}")
    assert worst_acc < 5.74e8
    assert worst_real <= 1


@pytest.mark.parametrize("fmt", R.FORMATS)
@pytest.mark.parametrize("matrix,full_range", R.TABLES)
def test_host_twin_on_unaligned_recordings(fmt, matrix, full_range):
    """N = 3, H = 50, W = 70: 5250 bytes a frame (no multiple of 16), 35 chroma columns; the recording starts 1 byte into a buffer."""
    N, H, W = 3, 50, 70
    assert inputs.yuv_frame_shape(H, W) == (75, 70)
    buf = np.random.default_rng(7).integers(0, 256, N * 75 * W + 1, dtype=np.uint8)
    frames = buf[1:].reshape(N, 75, W)
    got = inputs.yuv_to_rgb_host(frames, fmt, matrix, full_range)
    assert np.array_equal(got, R.to_rgb(frames, fmt, matrix, full_range))
    lead = inputs.yuv_to_rgb_host(frames.reshape(1, N, 75, W), fmt, matrix, full_range)      # any number of leading dimensions
    assert lead.shape == (1, N, H, W, 3) and np.array_equal(lead[0], got)
    one = inputs.yuv_to_rgb_host(frames[1], fmt, matrix, full_range)
    assert one.shape == (H, W, 3) and np.array_equal(one, got[1])


def test_layouts_differ_only_in_where_chroma_lies():
    rng = np.random.default_rng(3)
    H, W = 6, 8
    Y = rng.integers(0, 256, (H, W), dtype=np.uint8)
    U, V = rng.integers(0, 256, (2, H // 2, W // 2), dtype=np.uint8)
    nv12 = np.concatenate([Y, np.stack([U, V], axis=-1).reshape(H // 2, W)])
    i420 = np.concatenate([Y.reshape(-1), U.reshape(-1), V.reshape(-1)]).reshape(H * 3 // 2, W)
    a, b = inputs.yuv_to_rgb_host(nv12, "nv12"), inputs.yuv_to_rgb_host(i420, "i420")
    assert np.array_equal(a, b)
    # pixel (y, x) uses chroma (y >> 1, x >> 1): grey chroma everywhere but one sample colours exactly its 2 x 2 block
    flat = np.concatenate([np.full((H, W), 100, np.uint8), np.full((H // 2, W), 128, np.uint8)])
    flat[H + 1, 2 * 2] = 255                                                # U of chroma sample (1, 2)
    rgb = inputs.yuv_to_rgb_host(flat, "nv12")
    changed = (rgb != rgb[0, 0]).any(axis=-1)
    assert changed.sum() == 4 and changed[2:4, 4:6].all()


def test_abi_and_symbols():
    hdr = open(os.path.join(ROOT, "include", "csts_hip.h")).read()
    assert int(re.search(r"#define CSTS_ABI_VERSION (\d+)", hdr).group(1)) == lib.ABI_VERSION == 14
    assert re.search(r"CSTS_YUV_NV12 = 1, CSTS_YUV_I420 = 2", hdr) and (lib.YUV_NV12, lib.YUV_I420) == (1, 2)
    for path in lib._PATHS.values():
        handle = ctypes.CDLL(path)
        for name in NEW_SYMBOLS:
            assert hasattr(handle, name), (path, name)
            assert name in lib.SYMBOLS and re.search(r"\b" + name + r"\(", hdr)


def test_c_entry_points_refuse_bad_arguments_on_the_host():
    h = lib.load()
    x, o = np.zeros(3 * 8, np.uint8), np.zeros(4 * 4 * 3, np.uint8)
    ok = (x.ctypes.data, o.ctypes.data, 1, 4, 4)
    assert h.csts_yuv_to_rgb_host(*ok, lib.YUV_NV12, lib.YUV_BT601, 0) == 0
    assert h.csts_yuv_to_rgb_host(*ok, 0, lib.YUV_BT601, 0) == -1                 # rgb24 is no 4:2:0 layout
    assert h.csts_yuv_to_rgb_host(*ok, lib.YUV_I420, 2, 0) == -1                  # unknown matrix
    assert h.csts_yuv_to_rgb_host(x.ctypes.data, o.ctypes.data, 1, 3, 4, lib.YUV_NV12, 0, 0) == -1      # odd H
    assert b"even" in h.csts_last_error()
    assert h.csts_yuv_to_rgb_host(None, o.ctypes.data, 1, 4, 4, lib.YUV_NV12, 0, 0) == -1
    # the device entry points check their arguments before any launch
    f3 = (ctypes.c_float * 3)(1, 1, 1)
    assert h.csts_yuv_to_rgb(x.ctypes.data, o.ctypes.data, 1, 4, 5, lib.YUV_NV12, 0, 0, None) == -1   # odd W
    assert h.csts_spatial_sample_yuv(x.ctypes.data, x.ctypes.data, o.ctypes.data, 1, 1, 4, 6002, 4, f3, f3, 1, 0, 0, None) == -1
    assert h.csts_clip_sample_yuv(x.ctypes.data, 1, x.ctypes.data, x.ctypes.data, o.ctypes.data, 1, 1, 5, 4, 4, f3, f3, 1, 0, 0,
                                  None) == -1
    assert h.csts_batch_sample_yuv(x.ctypes.data, 24, x.ctypes.data, x.ctypes.data, x.ctypes.data, o.ctypes.data, 1, 1, 4, 4, f3, f3,
                                   3, 0, 0, None) == -1                            # unknown layout


def test_value_errors_come_before_the_device_check():
    """CPU tensors: every argument error is a ValueError; only a well-formed call reaches the "GPU only" error."""
    H, W, S = 8, 12, 4
    yuv5 = torch.zeros(1, 2, H * 3 // 2, W, dtype=torch.uint8)
    rgb5 = torch.zeros(1, 2, H, W, 3, dtype=torch.uint8)
    par = torch.tensor([[S, S, 0, 0, 0]], dtype=torch.int32)
    idx = torch.zeros(1, 2, dtype=torch.int32)
    lab = torch.zeros(1, 2, 2, dtype=torch.float64)
    assert inputs.PIXEL_FORMATS == ("rgb24", "nv12", "i420")
    with pytest.raises(ValueError, match="pixel_format"):
        inputs.spatial_sample(yuv5, par, S, pixel_format="yuv444")
    with pytest.raises(ValueError, match="matrix"):
        inputs.spatial_sample(yuv5, par, S, pixel_format="nv12", matrix="bt2020")
    # an odd H cannot be written as H * 3 / 2 rows: it shows as a row count that is no multiple of 3 (below), or in a clip table
    with pytest.raises(ValueError, match="even"):
        inputs.spatial_sample(torch.zeros(1, 2, 12, 7, dtype=torch.uint8), par, S, pixel_format="i420")      # odd W
    with pytest.raises(ValueError, match="multiple of 3"):
        inputs.spatial_sample(torch.zeros(1, 2, 10, 12, dtype=torch.uint8), par, S, pixel_format="nv12")
    with pytest.raises(ValueError):                                                  # a 4:2:0 shape passed as rgb24
        inputs.spatial_sample(yuv5, par, S)
    with pytest.raises(ValueError):                                                  # packed RGB passed as 4:2:0
        inputs.spatial_sample(rgb5, par, S, pixel_format="nv12")
    with pytest.raises(ValueError):
        inputs.clip_sample(rgb5[0], idx, par, S, pixel_format="i420")
    with pytest.raises(ValueError):
        inputs.clip_sample(yuv5[0], idx, par, S)
    with pytest.raises(ValueError, match="even"):
        inputs.clip_sample(torch.zeros(2, 12, 7, dtype=torch.uint8), idx, par, S, pixel_format="nv12")
    with pytest.raises(ValueError, match="pixel_format"):
        inputs.spatial_sampling(yuv5, lab, S, train=False, pixel_format="bgr")
    with pytest.raises(ValueError):
        inputs.spatial_sampling(rgb5, lab, S, train=False, pixel_format="nv12")
    with pytest.raises(ValueError, match="multiple of 3"):
        inputs.yuv_to_rgb(torch.zeros(2, 10, 12, dtype=torch.uint8), "nv12")
    with pytest.raises(ValueError, match="packed RGB"):
        inputs.yuv_to_rgb(rgb5, "nv12")
    with pytest.raises(ValueError):
        inputs.yuv_to_rgb(yuv5, "rgb24")
    with pytest.raises(ValueError, match="even"):
        inputs.yuv_frame_shape(5, 4)
    arena = torch.zeros(4096, dtype=torch.uint8)
    clips = torch.tensor([[1, 2, H, W]], dtype=torch.int64)
    with pytest.raises(ValueError, match="even"):
        inputs.batch_sample(arena, clips, idx, par, S, [[1, 2, 7, W]], pixel_format="nv12")
    with pytest.raises(ValueError, match="arena"):                                   # N H W 3 / 2 bytes from the offset on
        inputs.batch_sample(arena, clips, idx, par, S, [[4096 - 2 * H * W * 3 // 2 + 1, 2, H, W]], pixel_format="nv12")
    with pytest.raises(ValueError, match="pixel_format"):
        inputs.batch_sample(arena, clips, idx, par, S, [[1, 2, H, W]], pixel_format="p010")
    with pytest.raises(ValueError, match="pixel_format"):
        inputs.assemble_batch(yuv5, None, None, 1.0, lab, pixel_format="nv21")
    # well-formed calls get as far as the device check
    for call in (lambda: inputs.spatial_sample(yuv5, par, S, pixel_format="nv12"),
                 lambda: inputs.clip_sample(yuv5[0], idx, par, S, pixel_format="i420", matrix="bt709", full_range=True),
                 lambda: inputs.batch_sample(arena, clips, idx, par, S, [[1, 2, H, W]], pixel_format="nv12"),
                 lambda: inputs.yuv_to_rgb(yuv5, "i420")):
        with pytest.raises(lib.CstsError, match="MI355X only"):
            call()


def test_clip_pictures_reads_the_format_entries(tmp_path):
    from make_toy_dataset import write_dataset
    yuv = np.zeros((4, 9, 8), np.uint8)
    f, H, W, fmt = D.clip_pictures({"frames_yuv": yuv, "pixel_format": np.array("i420")}, "a.npz")
    assert (H, W, fmt) == (6, 8, ("i420", "bt601", False)) and f is yuv
    z = {"frames_yuv": yuv, "pixel_format": np.array("nv12"), "yuv_matrix": np.array("bt709"), "yuv_full_range": np.array(True)}
    assert D.clip_pictures(z, "a.npz")[3] == ("nv12", "bt709", True)
    assert D.clip_pictures(z, "a.npz", "i420", "bt601", False)[3] == ("i420", "bt601", False)      # the arguments override
    rgb = np.zeros((4, 6, 8, 3), np.uint8)
    assert D.clip_pictures({"frames_u8": rgb}, "a.npz")[1:] == (6, 8, ("rgb24", "bt601", False))
    # one clip of tools/predict.py --clip: (B, T, ...) pictures
    assert D.clip_pictures({"frames_u8": np.zeros((2, 4, 6, 8, 3), np.uint8)}, "a.npz", lead=2)[1:] == (6, 8, ("rgb24", "bt601", False))
    assert D.clip_pictures({"frames_yuv": np.zeros((2, 4, 9, 8), np.uint8), "pixel_format": np.array("nv12")}, "a.npz", lead=2)[1:3] == (6, 8)
    with pytest.raises(ValueError, match=r"\(B, T, H, W, 3\)"):
        D.clip_pictures({"frames_u8": rgb}, "a.npz", lead=2)
    with pytest.raises(ValueError, match="both frames_u8 and frames_yuv"):
        D.clip_pictures({"frames_u8": rgb, "frames_yuv": yuv, "pixel_format": np.array("nv12")}, "a.npz")
    with pytest.raises(ValueError, match="pixel_format"):
        D.clip_pictures({"frames_yuv": yuv}, "a.npz")
    with pytest.raises(ValueError, match="even"):
        D.clip_pictures({"frames_yuv": np.zeros((4, 9, 7), np.uint8), "pixel_format": np.array("nv12")}, "a.npz")
    # the toy writer: frames_yuv (N, H * 3 / 2, W) with a pixel_format entry, the rest of the data set as before
    out = str(tmp_path / "toy")
    write_dataset(out, clips_per_video=(1,), sizes=((36, 48),), test_clips=1, seed=1, pixel_format="nv12")
    with np.load(os.path.join(out, "clips", "video00", "video00_t0_t5.npz")) as z:
        assert "frames_u8" not in z.files and z["frames_yuv"].shape == (150, 54, 48) and str(z["pixel_format"]) == "nv12"
        assert D.clip_pictures(z, "toy")[3] == ("nv12", "bt601", False)
    with pytest.raises(ValueError, match="even"):
        write_dataset(str(tmp_path / "odd"), clips_per_video=(1,), sizes=((35, 48),), pixel_format="i420")
