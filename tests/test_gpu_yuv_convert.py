"""inputs.yuv_to_rgb (csts_yuv_to_rgb, csts_amd/csrc/yuv.hip) against the numpy int64 restatement of the colour rule
(tests/yuv_reference.py): equal, for both layouts and all four tables, on N = 3 frames of 50 x 70 (5250 bytes a frame: frames
start at bytes that are no multiple of 16; 35 chroma columns) preceded by an all-0 and followed by an all-255 frame, on that
recording starting 1 byte into a larger buffer, on a frame wider than one tile of the kernel, and into a given output, which
may itself start at any byte (a slice of a larger tensor)."""
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

import yuv_reference as R  # noqa: E402
from csts_amd import inputs  # noqa: E402

DEV = torch.device("cuda:0")
H, W = 50, 70


def _recording():
    rng = np.random.default_rng(17)
    body = rng.integers(0, 256, (3, H * 3 // 2, W), dtype=np.uint8)
    return np.concatenate([np.zeros_like(body[:1]), body, np.full_like(body[:1], 255)])


REC = _recording()                                                            # (5, 75, 70)
WANT = {(f, m, fr): R.to_rgb(REC, f, m, fr) for f in R.FORMATS for m, fr in R.TABLES}


@pytest.mark.parametrize("fmt", R.FORMATS)
@pytest.mark.parametrize("matrix,full_range", R.TABLES)
def test_device_equals_the_restatement(fmt, matrix, full_range):
    want = torch.from_numpy(WANT[(fmt, matrix, full_range)]).to(DEV)
    got = inputs.yuv_to_rgb(torch.from_numpy(REC).to(DEV), fmt, matrix, full_range)
    assert got.shape == (5, H, W, 3) and got.dtype == torch.uint8
    assert torch.equal(got, want)
    # the recording 1 byte into a larger buffer: every frame and every row starts at another alignment
    buf = torch.zeros(REC.size + 33, dtype=torch.uint8, device=DEV)
    buf[1:1 + REC.size] = torch.from_numpy(REC.reshape(-1)).to(DEV)
    view = buf[1:1 + REC.size].view(5, H * 3 // 2, W)
    assert view.data_ptr() % 16 == 1
    assert torch.equal(inputs.yuv_to_rgb(view, fmt, matrix, full_range), want)


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_leading_dimensions_out_and_wide_frames(fmt):
    x = torch.from_numpy(REC[:4]).to(DEV)
    want = torch.from_numpy(WANT[(fmt, "bt601", False)][:4]).to(DEV)
    got = inputs.yuv_to_rgb(x.view(2, 2, H * 3 // 2, W), fmt)
    assert got.shape == (2, 2, H, W, 3) and torch.equal(got.view(4, H, W, 3), want)
    assert torch.equal(inputs.yuv_to_rgb(x[1], fmt), want[1])
    out = torch.full((4, H, W, 3), 7, dtype=torch.uint8, device=DEV)
    assert inputs.yuv_to_rgb(x, fmt, out=out) is out and torch.equal(out, want)
    with pytest.raises(ValueError):
        inputs.yuv_to_rgb(x, fmt, out=out[:3])
    with pytest.raises(ValueError, match="share memory"):
        whole = torch.zeros(4 * H * W * 3, dtype=torch.uint8, device=DEV)
        inputs.yuv_to_rgb(whole[:x.numel()].view_as(x), fmt, out=whole.view(4, H, W, 3))
    # into a slice of a larger tensor that starts at no multiple of 16 bytes: 10500 bytes a picture, so picture 3 starts at byte
    # 31500 (= 12 mod 16); and at an odd byte of a flat buffer.  Nothing beside the slice is written.
    big = torch.full((7, H, W, 3), 9, dtype=torch.uint8, device=DEV)
    assert big[3:].data_ptr() % 16 == 12
    inputs.yuv_to_rgb(x, fmt, out=big[3:])
    assert torch.equal(big[3:], want) and bool((big[:3] == 9).all())
    flat = torch.full((4 * H * W * 3 + 64,), 9, dtype=torch.uint8, device=DEV)
    odd = flat[5:5 + 4 * H * W * 3].view(4, H, W, 3)
    assert odd.data_ptr() % 2 == 1
    inputs.yuv_to_rgb(x, fmt, out=odd)
    assert torch.equal(odd, want) and bool((flat[:5] == 9).all()) and bool((flat[5 + 4 * H * W * 3:] == 9).all())
    # wider than one tile of 1024 pixels, the last tile ragged: 2 frames of 6 x 2090
    wide = np.random.default_rng(5).integers(0, 256, (2, 9, 2090), dtype=np.uint8)
    got = inputs.yuv_to_rgb(torch.from_numpy(wide).to(DEV), fmt, "bt709", True)
    assert torch.equal(got, torch.from_numpy(R.to_rgb(wide, fmt, "bt709", True)).to(DEV))
