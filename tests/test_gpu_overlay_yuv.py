"""The overlay in 4:2:0 (csts_gaze_overlay_yuv, ops.gaze_overlay_yuv) and the device converter back (csts_rgb_to_yuv,
inputs.rgb_to_yuv), csts_amd/csrc/overlay.hip and yuv.hip.

rgb_to_yuv: equal to the host twin (tests/test_rgb_yuv_host.py pins that against the restated rule), bit for bit.

gaze_overlay_yuv: equal, byte for byte, to where(M, rgb_to_yuv(D), frames) (tests/rgb_yuv_reference.py::compose), M per pixel for
luma and per 2 x 2 block (any) for chroma.  D is the existing RGB op on yuv_to_rgb(frames) with the same arguments; M is the
existing RGB op drawn with alpha = 1 over all-black frames, "any channel non-zero" (JET is never black, the disc is green).  Both
come from kernels earlier tests pin, the encoding from the restated integer rule on the host: the reference is exact, there is no
tolerance.  Every case first asserts, on the reference, the property it is there for."""
import functools
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
from csts_amd import inputs, lib, ops  # noqa: E402

DEV = torch.device("cuda:0")

# name: N, H, W, S, params row, (mh, mw), centers (None: no markers), radius
CASES = {
    # rows 1..18 and columns 3..20 lie in the crop: every edge splits a 2 x 2 block.  A disc with an odd centre, one cut by the frame's
    # corner, and a frame with a negative centre X
    "crop_odd": (3, 20, 28, 16, [18, 25, 1, 3, 0], (4, 4), [[11, 9], [27, 19], [-1, 5]], 3),
    "no_centers": (2, 20, 28, 16, [18, 25, 1, 3, 0], (4, 4), None, 3),
    "one_block": (2, 2, 2, 2, [2, 2, 0, 0, 0], (1, 1), [[1, 1], [-1, 0]], 0),
    # 6 x 10: W = 2 (mod 4), 90 bytes a frame; the crop covers columns 2..7
    "w10": (4, 6, 10, 4, [5, 8, 0, 2, 0], (3, 5), [[4, 3], [9, 0], [-1, -1], [0, 5]], 2),
    # past any 1024-pixel tile: the crop covers columns 515..1029, a disc sits on column 1025
    "w1030": (2, 4, 1030, 4, [4, 8, 0, 4, 0], (3, 5), [[1025, 1], [3, 2]], 2),
    # two tiles of the kernel (W > 2048), the second ragged; the crop covers columns 1025..2049 and crosses the seam at 1040
    "w2050": (1, 4, 2050, 4, [4, 8, 0, 4, 0], (1, 1), [[1040, 2]], 3),
    # 19 row pairs: a second band of 3 pairs, whose last pass holds one pair; rows 3..33 in the crop
    "h38": (2, 38, 12, 16, [19, 16, 2, 0, 0], (64, 64), [[5, 31], [-3, 0]], 4),
    # the widest frame, W % 4 == 0: the vector kernel with more than 64 KB of LDS; the crop covers columns 3072..5119
    "w8192": (1, 2, 8192, 2, [2, 8, 0, 3, 0], (1, 1), [[8191, 1]], 2),
    # W = 2 (mod 4): the staged kernel, four tiles of 2048, and with the largest map more than 64 KB of LDS
    "w8190_bigmap": (1, 2, 8190, 2, [2, 8, 0, 3, 0], (90, 91), [[2047, 0]], 3),
    # the identity crop: every pixel of both frames is drawn, 64 x 64 maps
    "identity64": (2, 64, 64, 64, [64, 64, 0, 0, 0], (64, 64), [[63, 63], [10, 21]], 5),
}


def make_case(name):
    N, H, W, S, row, (mh, mw), centers, radius = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    frames = rng.integers(0, 256, (N, H * 3 // 2, W), dtype=np.uint8)
    maps = rng.random((N, mh, mw), dtype=np.float32)
    cen = None if centers is None else torch.tensor(centers, dtype=torch.int32, device=DEV)
    return frames, torch.from_numpy(maps).to(DEV), cen, row, S, radius


@functools.lru_cache(maxsize=None)
def reference(name, fmt, matrix="bt601", full_range=False, alpha=0.4):
    """want uint8 (N, H * 3 / 2, W), the mask M (N, H, W) and the per-block counts, computed once per case."""
    frames, maps, cen, row, S, radius = make_case(name)
    x = torch.from_numpy(frames).to(DEV)
    rgb = inputs.yuv_to_rgb(x, fmt, matrix, full_range)
    D = ops.gaze_overlay(rgb, maps, row, S, centers=cen, alpha=alpha, radius=radius).cpu().numpy()
    black = ops.gaze_overlay(torch.zeros_like(rgb), maps, row, S, centers=cen, alpha=1.0, radius=radius).cpu().numpy()
    M = (black != 0).any(axis=-1)
    want, cnt = Q.compose(frames, D, M, fmt, matrix, full_range)
    for a in (want, M, cnt):
        a.setflags(write=False)
    return want, M, cnt


def run(name, fmt, matrix="bt601", full_range=False, alpha=0.4, out=None, frames=None):
    f, maps, cen, row, S, radius = make_case(name)
    x = torch.from_numpy(f).to(DEV) if frames is None else frames
    return ops.gaze_overlay_yuv(x, maps, row, S, fmt, matrix, full_range, centers=cen, alpha=alpha, radius=radius, out=out)


def check_properties(name, fmt):
    """What each case is there for, asserted on the reference."""
    frames, _, cen, _, _, _ = make_case(name)
    want, M, cnt = reference(name, fmt)
    partial = (cnt >= 1) & (cnt <= 3)
    if name in ("crop_odd", "no_centers"):
        f = 0
        cols, rows = np.flatnonzero(M[f].any(axis=0)), np.flatnonzero(M[f].any(axis=1))
        if name == "no_centers":
            assert (cols[0], cols[-1], rows[0], rows[-1]) == (3, 20, 1, 18)         # odd left / top, even right / bottom edges
            assert (cnt == 4).any() and (cnt == 0).any()
        assert partial[f].any() and (cnt[f] == 1).any() and (cnt[f] == 2).any()
    if name == "crop_odd":
        assert M[0, 9, 11] and M[0, 6, 11] and not M[0, 19, 27]                       # the odd centre lies in the crop and is drawn
        assert M[1, 19, 27] and M[1, 16, 27] and M[1, 19, 24] and not M[1, 19, 23]    # cut by the corner, outside the crop
        assert not M[2].any() and np.array_equal(want[2], frames[2])                  # negative centre X: the source bytes
    if name == "one_block":
        assert cnt.shape == (2, 1, 1) and cnt[0, 0, 0] == 4 and cnt[1, 0, 0] == 0
    if name == "w10":
        assert partial.any() and not M[2].any() and M[1, 0, 9] and M[3, 5, 0]
    if name == "w1030":
        cols = np.flatnonzero(M[1].any(axis=0))
        assert M[0, 1, 1025] and cols[-1] == 1029 and 515 in cols and M[1, 2, 3]
    if name == "w2050":
        cols = np.flatnonzero(M[0].any(axis=0))
        assert cols[0] < 1040 <= cols[-1] and cols[-1] == 2049 and cols[0] % 2 == 1
    if name in ("w8192", "w8190_bigmap"):
        W = CASES[name][2]
        cols = np.flatnonzero(M[0, 1])
        heat = cols[(cols > 2100) & (cols < W - 10)]
        assert heat[0] > 3000 and heat[-1] > 5000 and heat[-1] - heat[0] + 1 == len(heat) and M[0].sum() > len(heat) * 2
        assert M[0, 1, 8191] if name == "w8192" else (M[0, 0, 2047] and M[0, 0, 2048] and M[0, 0, 2050] and not M[0, 0, 2051])
    if name == "h38":
        rows = np.flatnonzero(M[0].any(axis=1))
        assert rows[0] < 32 <= rows[-1] and rows[-1] < 36 and not M[0, 36:].any() and not M[1].any()
    if name == "identity64":
        assert M.all()                                                                # the identity crop draws every pixel
    return want, M, cnt


@pytest.mark.parametrize("fmt", Q.FORMATS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_equals_the_composition(name, fmt):
    want, M, cnt = check_properties(name, fmt)
    frames = torch.from_numpy(make_case(name)[0]).to(DEV)
    got = run(name, fmt, frames=frames)
    assert got.dtype == torch.uint8 and got.shape == frames.shape and got.data_ptr() != frames.data_ptr()
    g = got.cpu().numpy()
    bad = np.argwhere(g != want)
    assert bad.size == 0, (name, fmt, len(bad), bad[:8].tolist())
    assert np.array_equal(frames.cpu().numpy(), make_case(name)[0])                    # the input is not written
    # undrawn pixels and blocks carry their source bytes (part of `want`; stated on its own)
    Y0, U0, V0 = Q.split(make_case(name)[0], fmt)
    Y1, U1, V1 = Q.split(g, fmt)
    assert np.array_equal(Y1[~M], Y0[~M]) and np.array_equal(U1[cnt == 0], U0[cnt == 0]) and np.array_equal(V1[cnt == 0], V0[cnt == 0])


@pytest.mark.parametrize("fmt", Q.FORMATS)
@pytest.mark.parametrize("name", ["crop_odd", "w10", "h38", "w2050"])
def test_in_place_equals_out_of_place(name, fmt):
    want = reference(name, fmt)[0]
    work = torch.from_numpy(make_case(name)[0]).to(DEV)
    assert run(name, fmt, frames=work, out=work) is work
    assert np.array_equal(work.cpu().numpy(), want), (name, fmt)
    again = run(name, fmt)                                                             # and it is deterministic
    assert np.array_equal(again.cpu().numpy(), want)


@pytest.mark.parametrize("fmt", Q.FORMATS)
def test_a_chunk_of_a_recording_and_odd_addresses(fmt):
    """frames[1:3] of the 4-frame recording of 90-byte frames: the chunk starts at byte 90 (= 10 mod 16), in and out of place, into a
    chunk of a larger output; then the whole recording and its output 1 byte into their buffers.  Nothing else is written."""
    name = "w10"
    f, maps, cen, row, S, radius = make_case(name)
    want = reference(name, fmt)[0]
    rec = torch.from_numpy(f).to(DEV)
    assert rec[1:3].data_ptr() % 16 == 10
    kw = dict(centers=cen[1:3], radius=radius)
    got = ops.gaze_overlay_yuv(rec[1:3], maps[1:3], row, S, fmt, **kw)
    assert np.array_equal(got.cpu().numpy(), want[1:3])
    big = torch.full((4, 9, 10), 7, dtype=torch.uint8, device=DEV)
    assert ops.gaze_overlay_yuv(rec[1:3], maps[1:3], row, S, fmt, out=big[1:3], **kw).data_ptr() == big[1:3].data_ptr()
    assert np.array_equal(big[1:3].cpu().numpy(), want[1:3]) and bool((big[0] == 7).all()) and bool((big[3] == 7).all())
    work = rec.clone()
    ops.gaze_overlay_yuv(work[1:3], maps[1:3], row, S, fmt, out=work[1:3], **kw)       # in place, on the chunk alone
    assert np.array_equal(work[1:3].cpu().numpy(), want[1:3]) and torch.equal(work[0], rec[0]) and torch.equal(work[3], rec[3])
    src = torch.full((f.size + 3,), 9, dtype=torch.uint8, device=DEV)
    src[1:1 + f.size] = rec.flatten()
    dst = torch.full((f.size + 6,), 9, dtype=torch.uint8, device=DEV)
    a, b = src[1:1 + f.size].view(rec.shape), dst[3:3 + f.size].view(rec.shape)
    assert a.data_ptr() % 2 == 1 and b.data_ptr() % 2 == 1
    ops.gaze_overlay_yuv(a, maps, row, S, fmt, centers=cen, radius=radius, out=b)
    assert np.array_equal(b.cpu().numpy(), want) and bool((dst[:3] == 9).all()) and bool((dst[3 + f.size:] == 9).all())
    ops.gaze_overlay_yuv(a, maps, row, S, fmt, centers=cen, radius=radius, out=a)      # in place at an odd address
    assert np.array_equal(a.cpu().numpy(), want) and int(src[0]) == 9 and bool((src[1 + f.size:] == 9).all())


@pytest.mark.parametrize("fmt", Q.FORMATS)
@pytest.mark.parametrize("mh,mw", [(64, 64), (1, 1), (3, 5)])
def test_map_sizes(fmt, mh, mw):
    """64 x 64 (16-byte vector staging), 1 x 1 and 3 x 5 (15 cells: the maps of frames 1 and 2 start at no multiple of 16 bytes)."""
    f, _, cen, row, S, radius = make_case("crop_odd")
    maps = torch.from_numpy(np.random.default_rng(mh * 100 + mw).random((3, mh, mw), dtype=np.float32)).to(DEV)
    x = torch.from_numpy(f).to(DEV)
    rgb = inputs.yuv_to_rgb(x, fmt)
    D = ops.gaze_overlay(rgb, maps, row, S, centers=cen, radius=radius).cpu().numpy()
    want = Q.compose(f, D, reference("crop_odd", fmt)[1], fmt)[0]                      # the mask is geometry: that of the case
    got = ops.gaze_overlay_yuv(x, maps, row, S, fmt, centers=cen, radius=radius)
    assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("fmt", Q.FORMATS)
@pytest.mark.parametrize("alpha", [0.0, 0.4, 1.0])
def test_alphas(fmt, alpha):
    want, M, _ = reference("crop_odd", fmt, alpha=alpha)
    assert np.array_equal(M, reference("crop_odd", fmt)[1])                            # the mask does not depend on alpha
    got = run("crop_odd", fmt, alpha=alpha).cpu().numpy()
    assert np.array_equal(got, want)
    if alpha == 0.0:                                                                   # drawn pixels are re-encoded, not copied
        Y0 = Q.split(make_case("crop_odd")[0], fmt)[0]
        assert (Q.split(want, fmt)[0][M] != Y0[M]).any()


@pytest.mark.parametrize("fmt", Q.FORMATS)
@pytest.mark.parametrize("matrix,full_range", Q.TABLES)
def test_the_four_tables(fmt, matrix, full_range):
    want = reference("crop_odd", fmt, matrix, full_range)[0]
    assert np.array_equal(run("crop_odd", fmt, matrix, full_range).cpu().numpy(), want)
    if (matrix, full_range) != ("bt601", False):
        assert not np.array_equal(want, reference("crop_odd", fmt)[0])


def test_bad_params_on_the_device_draw_only_the_disc():
    """A params row that holds no crop, given as a device tensor (the kernel reads it): nothing is shaded, the disc is drawn."""
    f, maps, cen, _, S, radius = make_case("crop_odd")
    par = torch.tensor([18, 25, 9, 3, 0], dtype=torch.int32, device=DEV)                # y0 > nh - S
    x = torch.from_numpy(f).to(DEV)
    D = ops.gaze_overlay(inputs.yuv_to_rgb(x, "nv12"), maps, par, S, centers=cen, radius=radius).cpu().numpy()
    black = ops.gaze_overlay(torch.zeros(3, 20, 28, 3, dtype=torch.uint8, device=DEV), maps, par, S, centers=cen, alpha=1.0,
                             radius=radius).cpu().numpy()
    M = (black != 0).any(axis=-1)
    assert 0 < M.sum() < 60 and not M[2].any()
    want = Q.compose(f, D, M, "nv12")[0]
    assert np.array_equal(ops.gaze_overlay_yuv(x, maps, par, S, "nv12", centers=cen, radius=radius).cpu().numpy(), want)


def test_guards_return_an_error_and_write_nothing():
    h = lib.load()
    f, maps, cen, row, S, radius = make_case("crop_odd")
    x = torch.from_numpy(f).to(DEV)
    out = torch.full_like(x, 7)
    par = torch.tensor(row, dtype=torch.int32, device=DEV)
    wide = torch.zeros(1, 3, 8194, dtype=torch.uint8, device=DEV)
    wide_out = torch.full_like(wide, 7)

    def call(frames, o, N, H, W, mh=4, mw=4, layout=lib.YUV_NV12, matrix=0):
        return h.csts_gaze_overlay_yuv(frames, maps.data_ptr(), cen.data_ptr(), par.data_ptr(), o, N, H, W, S, mh, mw, 0.4, radius,
                                       layout, matrix, 0, None)

    assert call(x.data_ptr(), out.data_ptr(), 3, 19, 28) == -1 and b"even" in h.csts_last_error()          # odd H
    assert call(x.data_ptr(), out.data_ptr(), 3, 20, 27) == -1 and b"even" in h.csts_last_error()          # odd W
    assert call(wide.data_ptr(), wide_out.data_ptr(), 1, 2, 8194) == -1 and b"8192" in h.csts_last_error()
    assert call(x.data_ptr(), out.data_ptr(), 3, 20, 28, 128, 65) == -1 and b"MAX_HW" in h.csts_last_error()
    assert call(x.data_ptr(), out.data_ptr(), 3, 20, 28, layout=0) == -1
    assert call(x.data_ptr(), out.data_ptr(), 3, 20, 28, matrix=2) == -1
    assert call(x.data_ptr(), x.data_ptr() + 840, 2, 20, 28) == -1 and b"in place" in h.csts_last_error()  # frames[1:3] over [0:2]
    assert call(x.data_ptr(), None, 3, 20, 28) == -1
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((wide_out == 7).all()) and np.array_equal(x.cpu().numpy(), f)
    # the Python layer: the same refusals as exceptions
    with pytest.raises(lib.CstsError, match="MAX_HW"):
        ops.gaze_overlay_yuv(x, torch.zeros(3, 128, 65, device=DEV), row, S, "nv12", out=out)
    with pytest.raises(ValueError, match="in place"):
        ops.gaze_overlay_yuv(x[0:2], maps[0:2], row, S, "nv12", out=x[1:3])
    with pytest.raises(ValueError, match="even"):
        ops.gaze_overlay_yuv(torch.zeros(1, 9, 7, dtype=torch.uint8, device=DEV), maps[:1], row, S, "nv12")
    with pytest.raises(ValueError, match="gaze_overlay"):
        ops.gaze_overlay_yuv(x, maps, row, S, "rgb24")
    with pytest.raises(ValueError, match="out must"):
        ops.gaze_overlay_yuv(x, maps, row, S, "nv12", out=out[:2])
    torch.cuda.synchronize()
    assert bool((out == 7).all())


# ---- the converter back -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", Q.FORMATS)
@pytest.mark.parametrize("matrix,full_range", Q.TABLES)
def test_rgb_to_yuv_equals_the_host_twin(fmt, matrix, full_range):
    rng = np.random.default_rng(23)
    for N, H, W in ((1, 2, 2), (3, 6, 10), (2, 4, 1030), (2, 4, 2090)):               # 2090: three tiles of the kernel, the last ragged
        rgb = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
        want = inputs.rgb_to_yuv_host(rgb, fmt, matrix, full_range)
        got = inputs.rgb_to_yuv(torch.from_numpy(rgb).to(DEV), fmt, matrix, full_range)
        assert got.shape == (N, H * 3 // 2, W) and got.dtype == torch.uint8
        assert np.array_equal(got.cpu().numpy(), want), (H, W)


@pytest.mark.parametrize("fmt", Q.FORMATS)
def test_rgb_to_yuv_at_odd_addresses_and_into_a_given_output(fmt):
    N, H, W = 3, 6, 10
    rgb = np.random.default_rng(29).integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    want = inputs.rgb_to_yuv_host(rgb, fmt)
    src = torch.zeros(rgb.size + 1, dtype=torch.uint8, device=DEV)
    src[1:] = torch.from_numpy(rgb.reshape(-1)).to(DEV)
    x = src[1:].view(N, H, W, 3)
    flat = torch.full((N * 90 + 10,), 9, dtype=torch.uint8, device=DEV)
    out = flat[5:5 + N * 90].view(N, 9, W)
    assert x.data_ptr() % 2 == 1 and out.data_ptr() % 2 == 1
    assert inputs.rgb_to_yuv(x, fmt, out=out) is out
    assert np.array_equal(out.cpu().numpy(), want) and bool((flat[:5] == 9).all()) and bool((flat[5 + N * 90:] == 9).all())
    lead = inputs.rgb_to_yuv(x.view(1, N, H, W, 3), fmt)
    assert lead.shape == (1, N, 9, W) and np.array_equal(lead[0].cpu().numpy(), want)
    assert np.array_equal(inputs.rgb_to_yuv(x[1], fmt).cpu().numpy(), want[1])
    with pytest.raises(ValueError, match="share memory"):
        whole = torch.zeros(N * H * W * 3, dtype=torch.uint8, device=DEV)
        inputs.rgb_to_yuv(whole.view(N, H, W, 3), fmt, out=whole[:N * 90].view(N, 9, W))
    # the overlay in 4:2:0 against today's user path on a fully drawn picture: the same bytes
    f, maps, cen, row, S, radius = make_case("identity64")
    y = torch.from_numpy(f).to(DEV)
    D = ops.gaze_overlay(inputs.yuv_to_rgb(y, fmt), maps, row, S, centers=cen, radius=radius)
    assert torch.equal(ops.gaze_overlay_yuv(y, maps, row, S, fmt, centers=cen, radius=radius), inputs.rgb_to_yuv(D, fmt))
