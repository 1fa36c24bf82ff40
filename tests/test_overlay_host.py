"""The host side of the gaze overlay, no GPU: the JET table, the point and marker helpers, the argument checks of the C ABI, and
the seeded cases of tests/test_gpu_overlay.py held against their own cap on close pixels."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import overlay_reference as R  # noqa: E402


def test_jet_table_is_the_integer_formula():
    from csts_amd import jet_table, ops
    t = jet_table()
    assert t is not None and t.shape == (256, 3) and t.dtype == np.uint8 and ops.jet_table is jet_table
    assert tuple(t[0]) == (0, 0, 128) and tuple(t[255]) == (128, 0, 0) and t[128, 1] == 255
    for q in range(256):
        want = [min(max(383 - abs(4 * q - c), 0), 255) for c in (765, 510, 255)]
        assert t[q].tolist() == want, q
    assert np.array_equal(t, R.jet_formula(np.arange(256)))


def test_points_to_source_and_marker_centers():
    from csts_amd import marker_centers, points_to_source
    row, S, H, W = [32, 46, 0, 7, 0], 32, 36, 52          # 36 x 52 resized to 32 x 46, centre crop at x0 = 7
    pts = torch.tensor([[0.0, 0.0], [0.5, 0.25], [31 / 32, 31 / 32], [float("nan"), float("nan")]], dtype=torch.float32)
    src = points_to_source(pts, row, S)
    assert src.dtype == torch.float64 and src.shape == (4, 2)
    want = torch.tensor([[7 / 46, 0.0], [(16 + 7) / 46, 8 / 32], [(31 + 7) / 46, 31 / 32]], dtype=torch.float64)
    assert torch.allclose(src[:3], want, rtol=0, atol=1e-15) and bool(torch.isnan(src[3]).all())
    cen = marker_centers(src, H, W)
    assert cen.dtype == torch.int32 and cen.tolist() == [[7, 0], [26, 9], [42, 34], [-1, -1]]
    # the identity row leaves the points where they are
    assert torch.equal(points_to_source(pts[:3], [S, S, 0, 0, 0], S), pts[:3].double())
    with pytest.raises(ValueError):
        points_to_source(pts[:, :1], row, S)
    with pytest.raises(ValueError):
        marker_centers(src[0], H, W)


def test_bad_overlay_call_is_rejected_with_message_and_no_gpu_needed():
    from csts_amd import lib
    h = lib.load()
    buf = (C.c_uint8 * 64)()
    p = C.addressof(buf)
    assert h.csts_gaze_overlay(None, p, None, p, p, 1, 2, 2, 2, 1, 1, 0.4, 5, None) == -1
    assert b"csts_gaze_overlay" in h.csts_last_error() and b"NULL" in h.csts_last_error()
    assert h.csts_gaze_overlay(p, p, None, p, p, 0, 2, 2, 2, 1, 1, 0.4, 5, None) == -1
    assert b"csts_gaze_overlay" in h.csts_last_error() and b"N >= 1" in h.csts_last_error()
    assert h.csts_gaze_overlay(p, p, None, p, p, 1, 2, 2, 2, 1, 1, 1.5, 5, None) == -1 and b"alpha" in h.csts_last_error()
    assert h.csts_gaze_overlay(p, p, None, p, p, 1, 2, 2, 2, 1, 1, 0.4, -1, None) == -1 and b"radius" in h.csts_last_error()
    assert h.csts_gaze_overlay(p, p, None, p, p, 1, 2, 2, 2, 64, 129, 0.4, 5, None) == -1
    assert b"CSTS_GAZE_DECODE_MAX_HW" in h.csts_last_error()


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_seeded_cases_stay_under_the_cap_on_close_pixels(name):
    """The GPU test lets at most 1 % of the blended pixels be close to a quantisation step; the float64 reference of every
    seeded case must itself stay under that, and every case must have pixels inside and outside the crop as its row says."""
    H, W, S, mh, mw, idx = R.CASES[name]
    ref = R.case_reference(name)
    blended = int(ref["heat"].sum())
    assert blended > 0 and float(ref["close"].sum()) / blended <= 0.01
    assert not ref["heat"][1].any() and np.array_equal(ref["out"][1], R.make_case(name)["frames"][1].numpy())
    assert ref["marker"][0].sum() > 60 and 0 < ref["marker"][2].sum() < ref["marker"][0].sum()      # the corner disc is clipped
    if idx is None:
        assert ref["heat"][0].all()
    else:
        assert not ref["heat"][0].all()
        long_axis = 1 if W > H else 0
        assert ref["heat"][0].any(axis=long_axis).all()          # the short side is covered from edge to edge
