"""csts_gaze_overlay (csts_amd/csrc/overlay.hip, ops.gaze_overlay) against the rule of include/csts_hip.h restated in float64 on
the CPU (tests/overlay_reference.py).  cv2 is not installed, so the reference's own pixels are not what is compared.

Bound.  Outside the crop, on untouched frames (centre X < 0) and on marker pixels: equal.  Inside, a pixel is close when the
float64 v * 255 lies within 1e-3 of an integer: there the fp32 quantisation may land on the neighbouring q, one JET step of 4, and
at alpha 0.4 the output is off by at most 2 a channel.  Every other pixel is equal.  Close pixels are at most 1 % of the blended
ones (a cap; uniform chance gives 0.2 %, and tests/test_overlay_host.py holds the seeded cases to it on the CPU)."""
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

import overlay_reference as R  # noqa: E402
from csts_amd import jet_table, lib, ops  # noqa: E402

DEV = torch.device("cuda:0")


def dev_case(name):
    c = R.make_case(name)
    return c["frames"].to(DEV), c["maps"].to(DEV), c["centers"].to(DEV), c["row"], c["S"]


def unaligned(frames):
    """The same frames one byte into a buffer: no dword alignment, so the byte path."""
    buf = torch.empty(frames.numel() + 1, dtype=torch.uint8, device=DEV)
    buf[1:] = frames.flatten()
    un = buf[1:].view(frames.shape)
    assert un.data_ptr() % 4 != 0 and un.is_contiguous()
    return un


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_against_the_float64_rule(name):
    frames, maps, centers, row, S = dev_case(name)
    out = ops.gaze_overlay(frames, maps, row, S, centers=centers, radius=R.RADIUS)
    assert out.dtype == torch.uint8 and out.shape == frames.shape and out.data_ptr() != frames.data_ptr()
    R.compare(out, R.case_reference(name), name)
    assert torch.equal(frames.cpu(), R.make_case(name)["frames"])                      # the input is not written


def test_unaligned_frames_take_the_byte_path_and_give_the_same_bytes():
    frames, maps, centers, row, S = dev_case("landscape_idx1")
    vec = ops.gaze_overlay(frames, maps, row, S, centers=centers)
    byte = ops.gaze_overlay(unaligned(frames), maps, row, S, centers=centers)
    R.compare(byte, R.case_reference("landscape_idx1"), "landscape_idx1, frames one byte off")
    assert torch.equal(vec, byte)
    # an unaligned output alone also leaves the vector path
    out = unaligned(torch.zeros_like(frames))
    assert ops.gaze_overlay(frames, maps, row, S, centers=centers, out=out) is out and torch.equal(out, vec)


def test_in_place_equals_out_of_place_and_is_deterministic():
    for name in ("landscape_idx1", "byte_path_w50"):
        frames, maps, centers, row, S = dev_case(name)
        a = ops.gaze_overlay(frames, maps, row, S, centers=centers)
        b = ops.gaze_overlay(frames, maps, row, S, centers=centers)
        assert torch.equal(a, b)
        work = frames.clone()
        assert ops.gaze_overlay(work, maps, row, S, centers=centers, out=work) is work
        assert torch.equal(work, a), name


def test_alpha_zero_keeps_the_frames_and_alpha_one_shows_the_jet_table():
    name = "landscape_idx1"
    frames, maps, centers, row, S = dev_case(name)
    ref = R.case_reference(name)
    zero = ops.gaze_overlay(frames, maps, row, S, centers=centers, alpha=0.0).cpu().numpy()
    want = R.make_case(name)["frames"].numpy().copy()
    want[ref["marker"]] = (0, 255, 0)
    assert np.array_equal(zero, want)
    none = ops.gaze_overlay(frames, maps, row, S, centers=None, alpha=0.0)             # no markers at all: the frames
    assert torch.equal(none, frames)
    one = ops.gaze_overlay(frames, maps, row, S, centers=centers, alpha=1.0, radius=0).cpu().numpy()
    r1 = R.reference(R.make_case(name)["frames"], R.make_case(name)["maps"], R.make_case(name)["centers"], row, S, alpha=1.0, radius=0)
    assert int(r1["marker"].sum()) == 2                                               # radius 0: the centre pixel alone
    judged = r1["heat"] & ~r1["close"] & ~r1["marker"]
    assert judged.sum() > 0.98 * r1["heat"].sum()
    assert np.array_equal(one[judged], jet_table()[r1["q"][judged]])
    plain = R.make_case(name)["frames"].numpy()
    assert np.array_equal(one[~r1["heat"] & ~r1["marker"]], plain[~r1["heat"] & ~r1["marker"]])
    assert (one[r1["marker"]] == (0, 255, 0)).all()


def test_capturable_no_host_read():
    frames, maps, centers, row, S = dev_case("landscape_idx0")
    params = torch.tensor(row, dtype=torch.int32, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.gaze_overlay(frames, maps, params, S, centers=centers)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.gaze_overlay(frames, maps, params, S, centers=centers)              # a host read inside would fail the capture
    graph.replay()
    torch.cuda.synchronize()
    R.compare(out, R.case_reference("landscape_idx0"), "captured, landscape_idx0")
    # rescaled, centers and params rewritten between replays: the other crop, other maps, other markers
    other = R.make_case("landscape_idx2")
    maps.copy_(other["maps"].flip(0).to(DEV))
    centers.copy_(torch.tensor([[3, 30], [40, 12], [-1, -1]], dtype=torch.int32).to(DEV))
    params.copy_(torch.tensor(other["row"], dtype=torch.int32).to(DEV))
    assert other["row"] != row
    graph.replay()
    torch.cuda.synchronize()
    fresh = R.reference(R.make_case("landscape_idx0")["frames"], other["maps"].flip(0),
                        torch.tensor([[3, 30], [40, 12], [-1, -1]]), other["row"], S)
    R.compare(out, fresh, "replayed with rewritten rescaled, centers and params")


def test_arguments_are_validated():
    frames, maps, centers, row, S = dev_case("landscape_idx1")
    ok = dict(centers=centers)
    with pytest.raises(ValueError):
        ops.gaze_overlay(frames.float(), maps, row, S, **ok)
    with pytest.raises(ValueError):
        ops.gaze_overlay(frames, maps.double(), row, S, **ok)
    with pytest.raises(ValueError):
        ops.gaze_overlay(frames, maps, row, S, centers=centers.long())
    with pytest.raises(ValueError):
        ops.gaze_overlay(frames[0], maps, row, S, **ok)
    with pytest.raises(ValueError):
        ops.gaze_overlay(frames[..., :2], maps, row, S, **ok)
    with pytest.raises(ValueError):
        ops.gaze_overlay(frames, maps[:2], row, S, **ok)
    with pytest.raises(ValueError):
        ops.gaze_overlay(frames, maps, row, S, centers=centers[:2])
    with pytest.raises(ValueError):
        ops.gaze_overlay(frames, maps, row[:4], S, **ok)
    with pytest.raises(ValueError):
        ops.gaze_overlay(frames, maps, torch.tensor(row, dtype=torch.int64, device=DEV), S, **ok)
    with pytest.raises(ValueError, match="flip"):
        ops.gaze_overlay(frames, maps, row[:4] + [1], S, **ok)
    with pytest.raises(ValueError):
        ops.gaze_overlay(frames, maps, row, S, out=torch.empty(1, dtype=torch.uint8, device=DEV), **ok)
    for alpha in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="alpha"):
            ops.gaze_overlay(frames, maps, row, S, alpha=alpha, **ok)
    with pytest.raises(ValueError):
        ops.gaze_overlay(frames, maps, row, S, radius=-1, **ok)
    with pytest.raises(lib.CstsError):
        ops.gaze_overlay(frames.cpu(), maps, row, S, **ok)
    with pytest.raises(lib.CstsError):
        ops.gaze_overlay(frames, maps.cpu(), row, S, **ok)
    with pytest.raises(lib.CstsError):
        ops.gaze_overlay(frames, maps, torch.tensor(row, dtype=torch.int32), S, **ok)
    with pytest.raises(lib.CstsError, match="CSTS_GAZE_DECODE_MAX_HW"):
        ops.gaze_overlay(frames, torch.zeros(3, 64, 129, device=DEV), row, S, **ok)
